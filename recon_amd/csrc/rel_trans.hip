// RECON's per-relation translation residuals (models/models.py:939-958): for every entity pair m and every output relation r
//     s[m][r] = sum_d | tanh(head_m . W_r)_d + g_r,d - tanh(tail_m . W_r)_d |,   head, tail [M][ent_dim], W [n_rel][ent_dim][rel_dim], g [n_rel][rel_dim].
// The reference (and the op chain this replaces) writes both products, both tanh, the difference and its magnitude as [M][n_rel][rel_dim]
// tensors; here nothing of that size exists.
//
// k_rel_trans_fwd: one workgroup per (tile of 64 pairs, relation r), 4 waves, each wave 16 pairs.  A wave's 32-row A tile is its 16 head
//   rows on top of its 16 tail rows, so ONE B fragment of W_r feeds both sides, and in the 32x32 C/D layout (row = (reg & 3) + 8 (reg >> 2)
//   + 4 (lane >> 5), col = lane & 31) head row i sits in register q and tail row i in register q + 8 of the SAME lane: the epilogue — tanh,
//   + g_r, -, |.| — is lane-local.  The wave holds all of rel_dim as NS = ceil(rel_dim / 32) accumulator tiles (rel_dim <= 256), so the sum
//   over rel_dim is: per lane over its NS columns in slice order, then group_sum<32> over the 32 lanes: one fixed order, no atomics, no
//   second pass.  Products on v_mfma_f32_32x32x2_f32: exact fp32 fma chains in k order, no split planes to cache.  A comes through LDS
//   (k chunks of 64, zero-filled past M and past ent_dim: no alignment demanded of the row strides); W_r rows are read straight from
//   global memory (lane = column: 128-byte segments), four k ahead of the MFMAs that use them; the four waves of a workgroup and the
//   workgroups of one relation (adjacent in launch order) read the same 4 ent_dim rel_dim bytes.
//   For the backward it saves sgn(diff) in two bit planes (diff > 0, diff < 0): 2 NS words per (r, m), laid out [n_rel][M][NS][2], 1/16
//   of an fp32 intermediate.  Two planes because sgn(0) = 0 matters: a relation without a KB-GAT counterpart has W_r = 0 and g_r = 0, its
//   differences are exactly zero and its gradient must be.
// k_rel_trans_bwd: g_rel[r][d] = sum_m g_out[m][r] sgn(diff[m][r][d]).  One workgroup per relation, thread = (group of pairs, column d);
//   a group walks its pairs in increasing m, the groups are added in group order: fixed order, bitwise reproducible.
#include "prop_h_util.h"

namespace recon {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kRtPairs = 64;                 // pairs per workgroup (16 per wave)
constexpr int kRtKC = 64;                    // k chunk staged in LDS
constexpr int kRtLd = kRtKC + 1;             // odd pitch: the 32 rows a half-wave reads fall on 32 banks
constexpr int kRtMaxNS = 8;                  // rel_dim <= 256
constexpr int kRtBwdThreads = 1024;
constexpr int kRtRange = 0x7fffffff;        // range of the A descriptors: below kOOB, above every offset of a tile (row strides <= kRtMaxLd)
constexpr int64_t kRtMaxLd = 1 << 22;

// pair of the wave's 16 that C/D register q (0..7: head, q + 8: tail) of lane half lk holds
__device__ __forceinline__ int rt_pair_of(int q, int lk) { return (q & 3) + 8 * (q >> 2) + 4 * lk; }

template <int NS>
__global__ void __launch_bounds__(256, 2) k_rel_trans_fwd(const float* __restrict__ head, int64_t ld_head, const float* __restrict__ tail, int64_t ld_tail,
                                                       const float* __restrict__ W, const float* __restrict__ rel, int32_t M, int32_t n_rel,
                                                       int32_t ent_dim, int32_t rel_dim, float* __restrict__ out, uint32_t* __restrict__ saved) {
    __shared__ float As[2 * kRtPairs][kRtLd];                            // rows 32 w .. 32 w + 15: wave w's heads, + 16 .. 31: its tails
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6, lr = lane & 31, lk = lane >> 5;
    const int r = blockIdx.y, p0 = blockIdx.x * kRtPairs;
    // Every load below goes through a buffer descriptor and is masked by its ADDRESS (an offset past the range reads 0): a select on a
    // loaded value makes hipcc branch around each load and wait for it alone, one memory latency per element.
    const auto rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W + static_cast<int64_t>(r) * ent_dim * rel_dim), 0, ent_dim * rel_dim * 4, 0x00020000);
    const auto rG = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rel + static_cast<int64_t>(r) * rel_dim), 0, rel_dim * 4, 0x00020000);
    const auto rH = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(head + p0 * ld_head), 0, kRtRange, 0x00020000);     // this tile's rows; rows >= M and
    const auto rT = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(tail + p0 * ld_tail), 0, kRtRange, 0x00020000);     // k >= ent_dim masked below

    f32x16 acc[NS];
    uint32_t bcol[NS];                                                   // byte offset of this lane's column of slice s; past the range beyond rel_dim
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[s][q] = 0.f;
        const int c = 32 * s + lr;
        bcol[s] = c < rel_dim ? 4u * c : kOOB;
    }
    // B fragments of the k group [4 G, 4 G + 4): step e (0, 1) multiplies k = 4 G + 2 e + lk; rows k >= ent_dim lie past W_r: zeros
    auto load_b = [&](int G, float (&b)[2][NS]) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const uint32_t wk = static_cast<uint32_t>(4 * G + 2 * e + lk) * (4u * rel_dim);
#pragma unroll
            for (int s = 0; s < NS; ++s) b[e][s] = as_f(__builtin_amdgcn_raw_buffer_load_b32(rW, bcol[s] == kOOB ? kOOB : wk + bcol[s], 0, 0));
        }
    };
    auto mfma_group = [&](const float* a, const float (&b)[2][NS]) {      // k group at a[0 .. 3] of this lane's A row
        const float a0 = a[0], a1 = a[2];
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b[0][s], acc[s], 0, 0, 0);
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b[1][s], acc[s], 0, 0, 0);
    };
    float b0[2][NS], b1[2][NS];                                          // even / odd k groups (a chunk has an even number of them, the last aside)
    load_b(0, b0);

    const int wu = __builtin_amdgcn_readfirstlane(wid);                  // (tells the compiler that the staged row, and so head / tail, is wave-uniform)
    const float* arow = &As[32 * wid + lr][lk];
    const uint32_t ldh4 = 4u * static_cast<uint32_t>(ld_head), ldt4 = 4u * static_cast<uint32_t>(ld_tail);
    for (int k0 = 0; k0 < ent_dim; k0 += kRtKC) {
        const int kc = min(kRtKC, ent_dim - k0);
        if (k0) __syncthreads();                                         // the previous chunk has been read
        // element u of this thread: row 4 u + wave of As, column lane
        constexpr int kPer = 2 * kRtPairs * kRtKC / 256, kBatch = 16;    // elements per thread and chunk; loads in flight per thread
        static_assert(kRtKC == 64, "a wave stages one row of As per step");
        const uint32_t koff = lane < kc ? 4u * static_cast<uint32_t>(k0 + lane) : kOOB;
#pragma unroll 1
        for (int it0 = 0; it0 < kPer; it0 += kBatch) {
            float v[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int row = 4 * (it0 + u) + wu, i = row & 31, pl = 16 * (row >> 5) + (i & 15);
                const uint32_t roff = pl * (i < 16 ? ldh4 : ldt4);
                const uint32_t off = (p0 + pl < M && koff != kOOB) ? roff + koff : kOOB;
                v[u] = i < 16 ? as_f(__builtin_amdgcn_raw_buffer_load_b32(rH, off, 0, 0)) : as_f(__builtin_amdgcn_raw_buffer_load_b32(rT, off, 0, 0));
            }
#pragma unroll
            for (int u = 0; u < kBatch; ++u) As[4 * (it0 + u) + wu][lane] = v[u];
        }
        __syncthreads();
        const int ng = (kc + 3) >> 2, G = k0 >> 2;
        for (int g = 0; g < ng; g += 2) {                                // the next group's B rows are requested before this group's MFMAs
            load_b(G + g + 1, b1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_group(arow + 4 * g, b0);
            if (g + 1 < ng) {
                load_b(G + g + 2, b0);
                __builtin_amdgcn_sched_barrier(0);
                mfma_group(arow + 4 * g + 4, b1);
            }
        }
    }

    // epilogue on the accumulators.  Columns >= rel_dim: both products and g are 0 (masked loads): diff = 0, nothing added, sign 0.
    float part[8];
    uint32_t word[8];                                                    // lane lr < 2 NS: word lr (= 2 slice + plane) of pair rt_pair_of(q, lk)
#pragma unroll
    for (int q = 0; q < 8; ++q) { part[q] = 0.f; word[q] = 0u; }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const float gv = as_f(__builtin_amdgcn_raw_buffer_load_b32(rG, bcol[s], 0, 0));
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float hq = acc[s][q], tq = acc[s][q + 8];
            const float d = (tanh_fast(hq) + gv) - tanh_fast(tq);
            part[q] += fabsf(d);
            const unsigned long long pos = __ballot(d > 0.f), neg = __ballot(d < 0.f);
            const uint32_t wp = lk ? static_cast<uint32_t>(pos >> 32) : static_cast<uint32_t>(pos);
            const uint32_t wn = lk ? static_cast<uint32_t>(neg >> 32) : static_cast<uint32_t>(neg);
            if (lr == 2 * s) word[q] = wp;
            if (lr == 2 * s + 1) word[q] = wn;
        }
    }
    const int pw = p0 + 16 * wid;
    float mine = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float tot = group_sum<32>(part[q]);
        if (lr == q) mine = tot;
        const int m = pw + rt_pair_of(q, lk);
        if (saved && lr < 2 * NS && m < M) saved[(static_cast<int64_t>(r) * M + m) * (2 * NS) + lr] = word[q];
    }
    if (lr < 8) {
        const int m = pw + rt_pair_of(lr, lk);
        if (m < M) out[static_cast<int64_t>(m) * n_rel + r] = mine;
    }
}

__global__ void __launch_bounds__(kRtBwdThreads) k_rel_trans_bwd(const float* __restrict__ g_out, const uint32_t* __restrict__ saved, int32_t M,
                                                                 int32_t n_rel, int32_t rel_dim, int32_t ns, float* __restrict__ g_rel) {
    __shared__ float red[kRtBwdThreads];
    const int t = threadIdx.x, r = blockIdx.x;
    const int ncols = 32 * ns, groups = kRtBwdThreads / ncols, g = t / ncols, c = t - g * ncols;
    if (g < groups) {
        const uint2* sv = reinterpret_cast<const uint2*>(saved) + static_cast<int64_t>(r) * M * ns + (c >> 5);      // (pos, neg) of this column's slice
        const uint32_t bit = 1u << (c & 31);
        float acc = 0.f;
#pragma unroll 4
        for (int m = g; m < M; m += groups) {
            const uint2 w = sv[static_cast<int64_t>(m) * ns];
            const float go = g_out[static_cast<int64_t>(m) * n_rel + r];
            acc += go * (((w.x & bit) ? 1.f : 0.f) - ((w.y & bit) ? 1.f : 0.f));
        }
        red[t] = acc;
    }
    __syncthreads();
    if (t < rel_dim) {                                                   // rel_dim <= ncols: group 0's threads
        float sum = red[t];
        for (int gg = 1; gg < groups; ++gg) sum += red[gg * ncols + t];
        g_rel[static_cast<int64_t>(r) * rel_dim + t] = sum;
    }
}

template <int NS>
void rt_launch_fwd(dim3 grid, hipStream_t st, const float* head, int64_t ld_head, const float* tail, int64_t ld_tail, const float* W, const float* rel,
                   int32_t M, int32_t n_rel, int32_t ent_dim, int32_t rel_dim, float* out, uint32_t* saved) {
    hipLaunchKernelGGL(k_rel_trans_fwd<NS>, grid, dim3(256), 0, st, head, ld_head, tail, ld_tail, W, rel, M, n_rel, ent_dim, rel_dim, out, saved);
}

}  // namespace
}  // namespace recon

extern "C" int recon_rel_translation_supported(int64_t M, int32_t n_rel, int32_t ent_dim, int32_t rel_dim) {
    return M >= 1 && M <= (1 << 30) && n_rel >= 1 && n_rel <= 65535 && ent_dim >= 1 && ent_dim <= (1 << 20) && rel_dim >= 1 &&
           rel_dim <= 32 * recon::kRtMaxNS;
}

extern "C" size_t recon_rel_translation_saved_bytes(int64_t M, int32_t n_rel, int32_t rel_dim) {
    if (M <= 0 || n_rel <= 0 || rel_dim <= 0) return 0;
    return static_cast<size_t>(M) * static_cast<size_t>(n_rel) * static_cast<size_t>((rel_dim + 31) / 32) * 2 * sizeof(uint32_t);
}

extern "C" int recon_rel_translation_fwd(const float* head, int64_t ld_head, const float* tail, int64_t ld_tail, const float* W, const float* rel,
                                         int64_t M, int32_t n_rel, int32_t ent_dim, int32_t rel_dim, float* out, void* saved, recon_stream_t stream) {
    if (M < 0 || n_rel <= 0 || ent_dim <= 0 || rel_dim <= 0 || ld_head < 0 || ld_tail < 0) return RECON_ERR_INVALID;
    if (M == 0) return RECON_OK;
    if (!recon_rel_translation_supported(M, n_rel, ent_dim, rel_dim)) return RECON_ERR_UNSUPPORTED;
    if (!head || !tail || !W || !rel || !out) return RECON_ERR_INVALID;
    if (M > 1 && (ld_head < ent_dim || ld_tail < ent_dim)) return RECON_ERR_INVALID;
    if (ld_head > recon::kRtMaxLd || ld_tail > recon::kRtMaxLd) return RECON_ERR_UNSUPPORTED;
    const dim3 grid(static_cast<unsigned>((M + recon::kRtPairs - 1) / recon::kRtPairs), static_cast<unsigned>(n_rel));
    hipStream_t st = as_stream(stream);
    uint32_t* sv = static_cast<uint32_t*>(saved);
    const int32_t m = static_cast<int32_t>(M);
    switch ((rel_dim + 31) / 32) {
    case 1: recon::rt_launch_fwd<1>(grid, st, head, ld_head, tail, ld_tail, W, rel, m, n_rel, ent_dim, rel_dim, out, sv); break;
    case 2: recon::rt_launch_fwd<2>(grid, st, head, ld_head, tail, ld_tail, W, rel, m, n_rel, ent_dim, rel_dim, out, sv); break;
    case 3: recon::rt_launch_fwd<3>(grid, st, head, ld_head, tail, ld_tail, W, rel, m, n_rel, ent_dim, rel_dim, out, sv); break;
    case 4: recon::rt_launch_fwd<4>(grid, st, head, ld_head, tail, ld_tail, W, rel, m, n_rel, ent_dim, rel_dim, out, sv); break;
    case 5: recon::rt_launch_fwd<5>(grid, st, head, ld_head, tail, ld_tail, W, rel, m, n_rel, ent_dim, rel_dim, out, sv); break;
    case 6: recon::rt_launch_fwd<6>(grid, st, head, ld_head, tail, ld_tail, W, rel, m, n_rel, ent_dim, rel_dim, out, sv); break;
    case 7: recon::rt_launch_fwd<7>(grid, st, head, ld_head, tail, ld_tail, W, rel, m, n_rel, ent_dim, rel_dim, out, sv); break;
    default: recon::rt_launch_fwd<8>(grid, st, head, ld_head, tail, ld_tail, W, rel, m, n_rel, ent_dim, rel_dim, out, sv); break;
    }
    return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
}

extern "C" int recon_rel_translation_bwd(const float* g_out, const void* saved, int64_t M, int32_t n_rel, int32_t rel_dim, float* g_rel,
                                         recon_stream_t stream) {
    if (M < 0 || n_rel <= 0 || rel_dim <= 0) return RECON_ERR_INVALID;
    if (!recon_rel_translation_supported(M > 0 ? M : 1, n_rel, 1, rel_dim)) return RECON_ERR_UNSUPPORTED;
    if (!g_rel || (M > 0 && (!g_out || !saved))) return RECON_ERR_INVALID;
    hipLaunchKernelGGL(recon::k_rel_trans_bwd, dim3(static_cast<unsigned>(n_rel)), dim3(recon::kRtBwdThreads), 0, as_stream(stream), g_out,
                       static_cast<const uint32_t*>(saved), static_cast<int32_t>(M), n_rel, rel_dim, (rel_dim + 31) / 32, g_rel);
    return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
}
