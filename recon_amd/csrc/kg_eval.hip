// Link-prediction evaluation of the ConvKB scorer (GAT/layers.py:41-46 through SpKBGATConvOnly.batch_test, GAT/models.py:300-304), the scoring
// and ranking halves of Corpus.get_validation_pred (GAT/create_batch.py:905-1099) and get_validation_cnfmat (:1365-1420).
//
// fc1 acts on the concatenation [e_h; r; e_t], so with W1 = [W_h | W_r | W_t] it splits into three D x D projections computed once per
// evaluation (recon_sgemm_ex): P_h = E W_h^T, P_r = Rel W_r^T, P_t = E W_t^T.  A query (h, r, t) with one slot (column of the triple) replaced
// by candidate c then scores
//     s(q, c) = b2 + sum_d w2[d] * leaky(u[q, d] + P_slot[c, d]),      u[q] = (P_a[a] + P_b[b]) + b1
// where (a, b) are the two fixed columns in column order (head slot: r, t; relation slot: h, t; tail slot: h, r).  No GEMM is left for the
// candidates: a query side is a Q x N x D streaming VALU reduction.
//
// ONE score routine: every score this file produces — the true score s*, the scores counted in the tiled main loop, the scores of the filter
// correction and the dense scores — is the chain acc = fma(w2[d], leaky(u[d] + p[d]), acc) over d = 0, 1, ..., D - 1 from acc = 0, then
// acc + b2, with leaky(x) = max(x, slope x) (0 <= slope <= 1).  The same (query, candidate) therefore scores bit-identically on every path.
// (The tiled loop pads d up to a multiple of its chunk with zero u, p and w2: fma(0, 0, acc) = acc up to the sign of a zero, which compares
// equal.)
//
// Rank rule: rank = 1 + #{c not excluded by the query's filter : s(c) > s*}.  This is the position of the true triple in a stable descending
// sort with the true triple inserted at index 0 (GAT/create_batch.py:965-968, :1016-1020): ties are resolved in the true triple's favour.
//
// Kernels:
//   k_kge_prepare   one wave per query: writes u[q] to the workspace, s*[q], and rank[q] = 1 - #{excluded c : s(c) > s*} (the filter
//                   correction; the true id may be among the excluded ones, it does not count since its score equals s*)
//   k_kge_count     the main loop: a workgroup holds 64 queries and streams 64-candidate tiles of ITS candidate range through them in
//                   32-wide d chunks staged in LDS; every thread scores a 4 x 4 (query, candidate) block; the per-query counts are summed
//                   over the workgroup and added to rank[q] with one integer atomic (order-independent: deterministic)
//   k_kge_dense     S[q, j] = s(q, c0 + j), one thread per score (relation scores, test yardstick)
//
// The GAT_sep_space scorer carries both entities into the triple's relation space first, so its entity tables are per
// relation: P_h^r = tanh(E W_ent2rel[r]) W_h^T, P_t^r likewise with W_t (csrc/kg_sep.hip builds them for a chunk of Rc relations, [Rc][n][D]).
// The same score routine then runs on the table of the query's relation:
//   k_kgs_prepare   k_kge_prepare on queries sorted by relation; seg [Rc + 1] delimits each local relation's queries
//   k_kgs_count     k_kge_count on 64-query tiles that never cross a relation, each streaming ITS relation's candidate table
//   k_kgs_dense     S[q][rel_ids[rl]] = the relation-slot score on local relation rl's tables
// Both kernel pairs share the id check (kge_query), the prepare body (kge_prepare_query) and the count loop (kge_count_tiles); the flat
// kernels pass entity-table offset 0, the segmented ones the offset of the query's relation.
#include "recon_common.h"

#pragma clang fp contract(off)

namespace recon {
namespace {

constexpr int kQT = 64, kCT = 64, kDK = 32, kDKP = kDK + 4;    // query tile, candidate tile, d chunk, LDS row stride (36 / 4 odd: the 16
                                                                 // candidate rows a b128 lane group reads fall on distinct bank quads)
constexpr int kCountThreads = 256;
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float kge_leaky(float x, float slope) { return fmaxf(x, x * slope); }
__device__ __forceinline__ float kge_term(float acc, float u, float p, float w, float slope) { return fmaf(w, kge_leaky(u + p, slope), acc); }
__device__ __forceinline__ float kge_u(const float* pa, const float* pb, const float* b1, int d) { return (pa[d] + pb[d]) + b1[d]; }

struct KgeArgs {
    const int64_t* tri;     // [Q][3]
    const float* P[3];      // per column: P_h [n_ent, D], P_r [n_rel, D], P_t [n_ent, D]
    int64_t n[3];           // rows of P[k]
    const float* b1; const float* w2; const float* b2;
    int64_t Q; int32_t D, slot; float slope;
};

// the fixed columns of a slot, in column order
__device__ __forceinline__ void kge_fixed(int slot, int& ca, int& cb) {
    ca = slot == 0 ? 1 : 0;
    cb = slot == 2 ? 1 : 2;
}

// u rows of query q (pa, pb) and its true id; false when an id of q is outside its table.  ent_off offsets the entity tables P[0] and P[2]:
// 0 for the flat tables, rl n_ent D for local relation rl of per-relation tables [Rc][n_ent][D]
__device__ __forceinline__ bool kge_query(const KgeArgs& a, int64_t q, int64_t ent_off, const float*& pa, const float*& pb, int64_t& true_id) {
    int ca, cb;
    kge_fixed(a.slot, ca, cb);
    const int64_t ia = a.tri[3 * q + ca], ib = a.tri[3 * q + cb];
    true_id = a.tri[3 * q + a.slot];
    if (ia < 0 || ia >= a.n[ca] || ib < 0 || ib >= a.n[cb] || true_id < 0 || true_id >= a.n[a.slot]) return false;
    pa = a.P[ca] + (ca == 1 ? 0 : ent_off) + ia * a.D;
    pb = a.P[cb] + (cb == 1 ? 0 : ent_off) + ib * a.D;
    return true;
}

// the score routine (see the header comment): u computed on the fly, bit-identical to the workspace copy k_kge_prepare writes
__device__ float kge_score(const KgeArgs& a, const float* pa, const float* pb, const float* pc, float b2) {
    float acc = 0.f;
    for (int d = 0; d < a.D; ++d) acc = kge_term(acc, kge_u(pa, pb, a.b1, d), pc[d], a.w2[d], a.slope);
    return acc + b2;
}

// one query of the prepare pass (head or tail slot): u[q] to the workspace, s*[q], and the filter correction in rank[q]
__device__ __forceinline__ void kge_prepare_query(const KgeArgs& a, int64_t q, int64_t ent_off, const int64_t* __restrict__ filt_ids,
                                                  const int64_t* __restrict__ filt_begin, const int64_t* __restrict__ filt_end, float* __restrict__ U,
                                                  int64_t* __restrict__ rank, float* __restrict__ true_score) {
    const int lane = threadIdx.x;
    const float* pa; const float* pb; int64_t tid;
    float* uq = U + q * a.D;
    if (!kge_query(a, q, ent_off, pa, pb, tid)) {                         // bad id: rank 0, s* NaN (the count pass then adds nothing)
        for (int d = lane; d < a.D; d += kWave) uq[d] = 0.f;
        if (lane == 0) { rank[q] = 0; true_score[q] = __builtin_nanf(""); }
        return;
    }
    for (int d = lane; d < a.D; d += kWave) uq[d] = kge_u(pa, pb, a.b1, d);
    const float b2 = a.b2[0];
    const float* Pc = a.P[a.slot] + ent_off;
    const int64_t nc = a.n[a.slot];
    const float s_true = kge_score(a, pa, pb, Pc + tid * a.D, b2);
    int cnt = 0;
    if (filt_ids) {
        const int64_t e = filt_end[q];
        for (int64_t k = filt_begin[q] + lane; k < e; k += kWave) {
            const int64_t c = filt_ids[k];
            if (c >= 0 && c < nc && kge_score(a, pa, pb, Pc + c * a.D, b2) > s_true) ++cnt;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) { rank[q] = 1 - cnt; true_score[q] = s_true; }
}

__global__ void __launch_bounds__(64) k_kge_prepare(const KgeArgs a, const int64_t* __restrict__ filt_ids, const int64_t* __restrict__ filt_begin,
                                                    const int64_t* __restrict__ filt_end, float* __restrict__ U, int64_t* __restrict__ rank,
                                                    float* __restrict__ true_score) {
    kge_prepare_query(a, blockIdx.x, 0, filt_ids, filt_begin, filt_end, U, rank, true_score);
}

// stage rows [r0, r0 + 64) x [d0, d0 + 32) of a [rows, D] table into LDS (zeros outside): thread t moves column t % 32 of rows t / 32 + 8 k
__device__ __forceinline__ void kge_stage(float (*dst)[kDKP], const float* __restrict__ src, int64_t r0, int64_t rows, int D, int d0) {
    constexpr int kStep = kCountThreads / kDK;
    const int r = threadIdx.x / kDK, c = threadIdx.x % kDK;
    const int64_t row = r0 + r;
    const bool col_ok = d0 + c < D;
    const float* p = src + row * D + d0 + c;
    const int64_t step = static_cast<int64_t>(kStep) * D;
#pragma unroll
    for (int k = 0; k < kQT / kStep; ++k) dst[r + kStep * k][c] = (col_ok && row + kStep * k < rows) ? p[k * step] : 0.f;
}

// the main loop of the count pass: queries [q0, q0 + 64) below q_end (their u rows in U) against the candidate
// tiles [t_begin, t_end) of Pc [nc][D]; each query's count of candidates scoring above its s* is added to rank[q]
__device__ __forceinline__ void kge_count_tiles(const KgeArgs& a, float (*us)[kDKP], float (*ps)[kDKP], float* ws, const float* __restrict__ U,
                                                const float* __restrict__ true_score, int64_t* __restrict__ rank, int64_t q0, int64_t q_end,
                                                const float* __restrict__ Pc, int64_t nc, int64_t t_begin, int64_t t_end) {
    const int tq = threadIdx.x / 16, tc = threadIdx.x % 16;              // queries tq + 16 i, candidates tc + 16 j of the tile
    const int D = a.D;
    const float b2 = a.b2[0];
    float s_true[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t q = q0 + tq + 16 * i;
        s_true[i] = q < q_end ? true_score[q] : __builtin_nanf("");       // padding queries: NaN, nothing compares above it
    }
    int cnt[4] = {0, 0, 0, 0};
    for (int64_t tile = t_begin; tile < t_end; ++tile) {
        const int64_t c0 = tile * kCT;
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
        for (int d0 = 0; d0 < D; d0 += kDK) {
            __syncthreads();                                              // the previous chunk's readers are done
            kge_stage(us, U, q0, q_end, D, d0);
            kge_stage(ps, Pc, c0, nc, D, d0);
            if (threadIdx.x < kDK) ws[threadIdx.x] = d0 + static_cast<int>(threadIdx.x) < D ? a.w2[d0 + threadIdx.x] : 0.f;
            __syncthreads();
            for (int dd = 0; dd < kDK; dd += 4) {
                float4 u4[4], p4[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) u4[i] = *reinterpret_cast<const float4*>(&us[tq + 16 * i][dd]);
#pragma unroll
                for (int j = 0; j < 4; ++j) p4[j] = *reinterpret_cast<const float4*>(&ps[tc + 16 * j][dd]);
                const float4 w4 = *reinterpret_cast<const float4*>(&ws[dd]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        // u + p and slope (u + p) for d pairs as packed fp32 ops (per lane IEEE: the values kge_term computes)
                        const f32x2 x0 = f32x2{u4[i].x, u4[i].y} + f32x2{p4[j].x, p4[j].y}, x1 = f32x2{u4[i].z, u4[i].w} + f32x2{p4[j].z, p4[j].w};
                        const f32x2 m0 = x0 * a.slope, m1 = x1 * a.slope;
                        float v = acc[i][j];
                        v = fmaf(w4.x, fmaxf(x0.x, m0.x), v);
                        v = fmaf(w4.y, fmaxf(x0.y, m0.y), v);
                        v = fmaf(w4.z, fmaxf(x1.x, m1.x), v);
                        v = fmaf(w4.w, fmaxf(x1.y, m1.y), v);
                        acc[i][j] = v;
                    }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + tc + 16 * j < nc)
#pragma unroll
                for (int i = 0; i < 4; ++i) cnt[i] += (acc[i][j] + b2) > s_true[i];
    }
    // sum over the 16 threads of a query row (lanes tc = 0..15 of one 16-lane group), one atomic per query and workgroup
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int c = cnt[i];
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) c += __shfl_xor(c, o, 16);
        const int64_t q = q0 + tq + 16 * i;
        if (tc == 0 && q < q_end && c != 0) atomicAdd(reinterpret_cast<unsigned long long*>(rank + q), static_cast<unsigned long long>(c));
    }
}

__global__ void __launch_bounds__(kCountThreads) k_kge_count(const KgeArgs a, const float* __restrict__ U, const float* __restrict__ true_score,
                                                             int64_t* __restrict__ rank, int64_t tiles_per_split) {
    __shared__ float us[kQT][kDKP], ps[kCT][kDKP], ws[kDK];
    const int64_t nc = a.n[a.slot];
    const int64_t n_tiles = (nc + kCT - 1) / kCT;
    const int64_t t_begin = static_cast<int64_t>(blockIdx.y) * tiles_per_split;
    const int64_t t_end = t_begin + tiles_per_split < n_tiles ? t_begin + tiles_per_split : n_tiles;
    kge_count_tiles(a, us, ps, ws, U, true_score, rank, static_cast<int64_t>(blockIdx.x) * kQT, a.Q, a.P[a.slot], nc, t_begin, t_end);
}

__global__ void __launch_bounds__(256) k_kge_dense(const KgeArgs a, int64_t c0, int64_t C, float* __restrict__ S, int64_t ldS) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x, q = blockIdx.y;
    if (j >= C) return;
    const float* pa; const float* pb; int64_t tid;
    const int64_t c = c0 + j;
    float s = __builtin_nanf("");
    if (kge_query(a, q, 0, pa, pb, tid) && c >= 0 && c < a.n[a.slot]) s = kge_score(a, pa, pb, a.P[a.slot] + c * a.D, a.b2[0]);
    S[q * ldS + j] = s;
}

// ---- relation-segmented passes of the GAT_sep_space scorer ----
// the local relation of query q: seg[j] <= q < seg[j + 1] (seg non-decreasing, seg[0] = 0, seg[Rc] = Q; any seg stays inside [0, Rc))
__device__ __forceinline__ int kgs_segment(const int64_t* __restrict__ seg, int Rc, int64_t q) {
    int lo = 0, hi = Rc;
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (seg[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(64) k_kgs_prepare(const KgeArgs a, const int64_t* __restrict__ seg, int Rc, const int64_t* __restrict__ filt_ids,
                                                    const int64_t* __restrict__ filt_begin, const int64_t* __restrict__ filt_end, float* __restrict__ U,
                                                    int64_t* __restrict__ rank, float* __restrict__ true_score) {
    const int64_t q = blockIdx.x;
    const int64_t ent_off = static_cast<int64_t>(kgs_segment(seg, Rc, q)) * a.n[0] * a.D;
    kge_prepare_query(a, q, ent_off, filt_ids, filt_begin, filt_end, U, rank, true_score);
}

// grid.x: the bound ceil(Q / 64) + Rc on the number of 64-query tiles that never cross a relation; a workgroup finds its tile by walking the
// segments (Rc is a few dozen) and leaves when it has none
__global__ void __launch_bounds__(kCountThreads) k_kgs_count(const KgeArgs a, const int64_t* __restrict__ seg, int Rc, const float* __restrict__ U,
                                                             const float* __restrict__ true_score, int64_t* __restrict__ rank, int64_t tiles_per_split) {
    __shared__ float us[kQT][kDKP], ps[kCT][kDKP], ws[kDK];
    __shared__ int64_t tile[3];                                           // local relation, first query, end of the relation's queries
    if (threadIdx.x == 0) {
        int64_t b = blockIdx.x, rl = -1, q0 = 0, q_end = 0;
        for (int j = 0; j < Rc; ++j) {
            const int64_t s0 = seg[j], s1 = seg[j + 1], nt = s1 > s0 ? (s1 - s0 + kQT - 1) / kQT : 0;
            if (b < nt) { rl = j; q0 = s0 + b * kQT; q_end = s1; break; }
            b -= nt;
        }
        if (q0 < 0 || q_end > a.Q) rl = -1;                               // a malformed seg reads nothing outside the workspace
        tile[0] = rl; tile[1] = q0; tile[2] = q_end;
    }
    __syncthreads();
    const int64_t rl = tile[0], q0 = tile[1], q_end = tile[2];
    if (rl < 0) return;
    const int64_t nc = a.n[a.slot];
    const int64_t n_tiles = (nc + kCT - 1) / kCT;
    const int64_t t_begin = static_cast<int64_t>(blockIdx.y) * tiles_per_split;
    const int64_t t_end = t_begin + tiles_per_split < n_tiles ? t_begin + tiles_per_split : n_tiles;
    kge_count_tiles(a, us, ps, ws, U, true_score, rank, q0, q_end, a.P[a.slot] + rl * nc * a.D, nc, t_begin, t_end);
}

// S[q][rel_ids[rl]] = s(q with relation rel_ids[rl]) on local relation rl's entity tables: one thread per (query, local relation)
__global__ void __launch_bounds__(256) k_kgs_dense(const KgeArgs a, const int64_t* __restrict__ rel_ids, int Rc, float* __restrict__ S, int64_t ldS) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= a.Q * Rc) return;
    const int64_t q = i / Rc;
    const int rl = static_cast<int>(i % Rc);
    const int64_t c = rel_ids[rl];
    if (c < 0 || c >= ldS) return;
    const float* pa; const float* pb; int64_t tid;
    float s = __builtin_nanf("");
    if (kge_query(a, q, static_cast<int64_t>(rl) * a.n[0] * a.D, pa, pb, tid) && c < a.n[1]) s = kge_score(a, pa, pb, a.P[1] + c * a.D, a.b2[0]);
    S[q * ldS + c] = s;
}

int kge_args(KgeArgs& a, int32_t slot, int64_t Q, const int64_t* triples, const float* P_h, const float* P_r, const float* P_t, int64_t n_ent,
             int64_t n_rel, int32_t D, const float* b1, const float* w2, const float* b2, float slope) {
    if (slot < 0 || slot > 2 || Q < 0 || D < 1 || n_ent < 1 || n_rel < 1) return RECON_ERR_INVALID;
    if (!(slope >= 0.f && slope <= 1.f)) return RECON_ERR_UNSUPPORTED;     // leaky(x) = max(x, slope x) holds on [0, 1]
    if (Q > 0x7fffffffLL || n_ent > 0x7fffffffLL) return RECON_ERR_UNSUPPORTED;
    if (!triples || !P_h || !P_r || !P_t || !b1 || !w2 || !b2) return RECON_ERR_INVALID;
    a.tri = triples;
    a.P[0] = P_h; a.P[1] = P_r; a.P[2] = P_t;
    a.n[0] = n_ent; a.n[1] = n_rel; a.n[2] = n_ent;
    a.b1 = b1; a.w2 = w2; a.b2 = b2;
    a.Q = Q; a.D = D; a.slot = slot; a.slope = slope;
    return RECON_OK;
}

// the count pass's grid: q_tiles query tiles (grid.x) times a split of the nc candidates (grid.y) such that about 2048 workgroups (8 per CU)
// are in flight; per: candidate tiles per split
dim3 kge_count_grid(int64_t q_tiles, int64_t nc, int64_t& per) {
    const int64_t c_tiles = ceil_div64(nc, kCT);
    int64_t splits = ceil_div64(2048, q_tiles);
    if (splits > c_tiles) splits = c_tiles;
    per = ceil_div64(c_tiles, splits);
    splits = ceil_div64(c_tiles, per);
    return dim3(static_cast<unsigned>(q_tiles), static_cast<unsigned>(splits));
}

}  // namespace
}  // namespace recon

extern "C" size_t recon_convkb_rank_workspace_floats(int64_t Q, int32_t D) {
    return Q > 0 && D > 0 ? static_cast<size_t>(Q) * static_cast<size_t>(D) : 0;
}

extern "C" int recon_convkb_rank(int32_t slot, int64_t Q, const int64_t* triples, const float* P_h, const float* P_r, const float* P_t,
                                 int64_t n_ent, int64_t n_rel, int32_t D, const float* b1, const float* w2, const float* b2, float slope,
                                 const int64_t* filt_ids, const int64_t* filt_begin, const int64_t* filt_end, float* workspace,
                                 size_t workspace_floats, int64_t* ranks, float* true_scores, recon_stream_t stream) {
    recon::KgeArgs a;
    const int st = recon::kge_args(a, slot, Q, triples, P_h, P_r, P_t, n_ent, n_rel, D, b1, w2, b2, slope);
    if (st != RECON_OK) return st;
    if (filt_ids && (!filt_begin || !filt_end)) return RECON_ERR_INVALID;
    if (Q == 0) return RECON_OK;
    if (!ranks || !true_scores || !workspace) return RECON_ERR_INVALID;
    if (workspace_floats < recon_convkb_rank_workspace_floats(Q, D)) return RECON_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(recon::k_kge_prepare, dim3(static_cast<unsigned>(Q)), dim3(recon::kWave), 0, s, a, filt_ids, filt_begin, filt_end, workspace,
                       ranks, true_scores);
    RECON_CHECK_LAUNCH();
    int64_t per;
    const dim3 grid = recon::kge_count_grid(ceil_div64(Q, recon::kQT), a.n[slot], per);
    hipLaunchKernelGGL(recon::k_kge_count, grid, dim3(recon::kCountThreads), 0, s, a, workspace, true_scores, ranks, per);
    return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
}

extern "C" int recon_convkb_scores(int32_t slot, int64_t Q, const int64_t* triples, const float* P_h, const float* P_r, const float* P_t,
                                   int64_t n_ent, int64_t n_rel, int32_t D, const float* b1, const float* w2, const float* b2, float slope, int64_t c0,
                                   int64_t C, float* S, int64_t ldS, recon_stream_t stream) {
    recon::KgeArgs a;
    const int st = recon::kge_args(a, slot, Q, triples, P_h, P_r, P_t, n_ent, n_rel, D, b1, w2, b2, slope);
    if (st != RECON_OK) return st;
    if (C < 0 || c0 < 0 || c0 + C > a.n[slot] || ldS < C) return RECON_ERR_INVALID;
    if (Q == 0 || C == 0) return RECON_OK;
    if (!S) return RECON_ERR_INVALID;
    if (Q > 65535) return RECON_ERR_UNSUPPORTED;                          // grid.y: the caller chunks the queries
    hipLaunchKernelGGL(recon::k_kge_dense, dim3(static_cast<unsigned>(ceil_div64(C, 256)), static_cast<unsigned>(Q)), dim3(256), 0, as_stream(stream),
                       a, c0, C, S, ldS);
    return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
}

extern "C" int recon_kgsep_rank(int32_t slot, int64_t Q, const int64_t* triples, const int64_t* seg, int32_t Rc, const float* P_h, const float* P_r,
                                const float* P_t, int64_t n_ent, int64_t n_rel, int32_t D, const float* b1, const float* w2, const float* b2, float slope,
                                const int64_t* filt_ids, const int64_t* filt_begin, const int64_t* filt_end, float* workspace, size_t workspace_floats,
                                int64_t* ranks, float* true_scores, recon_stream_t stream) {
    recon::KgeArgs a;
    const int st = recon::kge_args(a, slot, Q, triples, P_h, P_r, P_t, n_ent, n_rel, D, b1, w2, b2, slope);
    if (st != RECON_OK) return st;
    if (slot == RECON_KGE_RELATION || Rc < 1 || !seg || (filt_ids && (!filt_begin || !filt_end))) return RECON_ERR_INVALID;
    if (Q == 0) return RECON_OK;
    if (!ranks || !true_scores || !workspace) return RECON_ERR_INVALID;
    if (workspace_floats < recon_convkb_rank_workspace_floats(Q, D)) return RECON_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(recon::k_kgs_prepare, dim3(static_cast<unsigned>(Q)), dim3(recon::kWave), 0, s, a, seg, Rc, filt_ids, filt_begin, filt_end,
                       workspace, ranks, true_scores);
    RECON_CHECK_LAUNCH();
    const int64_t q_tiles = ceil_div64(Q, recon::kQT) + Rc;              // the tile bound of k_kgs_count
    if (q_tiles > 0x7fffffffLL) return RECON_ERR_UNSUPPORTED;
    int64_t per;
    const dim3 grid = recon::kge_count_grid(q_tiles, n_ent, per);
    hipLaunchKernelGGL(recon::k_kgs_count, grid, dim3(recon::kCountThreads), 0, s, a, seg, Rc, workspace, true_scores, ranks, per);
    return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
}

extern "C" int recon_kgsep_scores(int64_t Q, const int64_t* triples, const int64_t* rel_ids, int32_t Rc, const float* P_h, const float* P_r,
                                  const float* P_t, int64_t n_ent, int64_t n_rel, int32_t D, const float* b1, const float* w2, const float* b2, float slope,
                                  float* S, int64_t ldS, recon_stream_t stream) {
    recon::KgeArgs a;
    const int st = recon::kge_args(a, RECON_KGE_RELATION, Q, triples, P_h, P_r, P_t, n_ent, n_rel, D, b1, w2, b2, slope);
    if (st != RECON_OK) return st;
    if (Rc < 1 || !rel_ids || ldS < n_rel) return RECON_ERR_INVALID;
    if (Q == 0) return RECON_OK;
    if (!S) return RECON_ERR_INVALID;
    const int64_t blocks = ceil_div64(Q * Rc, 256);
    if (blocks > 0x7fffffffLL) return RECON_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(recon::k_kgs_dense, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, as_stream(stream), a, rel_ids, Rc, S, ldS);
    return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
}
