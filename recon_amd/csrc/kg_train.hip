// Training of the ConvKB scorer over frozen embedding tables: stage B of KB-GAT, train_conv (GAT/main.py:707-860).
//
// Corruption (k_kgt_corrupt): the negative half of Corpus.get_iteration_batch (GAT/create_batch.py:103-260) and of
// get_iteration_triples_batch (:262-351).  Output row o < B is positive o; row B + c (c < 2 B r) starts as a copy of positive c mod B (the
// np.tile) and replaces
//     the head      for c in [0, B (r/2)),
//     the tail      for c in [B (r/2), 2 B (r/2)),
//     the relation  for c in [B r, 2 B r);
// for odd r the rows c in [2 B (r/2), B r) stay untouched copies.  A replaced row has value -1.  Entity draws are uniform over [0, n_ent)
// and redrawn while the triple is a known one (the reference's unbounded while); after kEntityDrawCap draws the row stays an untouched copy
// and a device counter is incremented.  Relation draws follow the reference's give-up rule: at most n_rel membership checks, then the row
// keeps the positive's relation and value.  Membership is a binary search in sorted unique int64 keys (r n_ent + h) n_ent + t.
// Draw k of row c is mix(seed, c, k) (splitmix64 finaliser, range by the high half of a 64 x 64 product): one thread per row, and the
// output depends on (seed, inputs) only, never on the launch shape.
//
// Scorer: X_m = [E[h_m] | Rel[r_m] | E[t_m]] (K = 3 D, read in place from the tables, never copied), z = X W1^T + b1, h1 = leaky(z) with
// leaky(x) = max(x, slope x) (nl1: 0.01), s = h1 . w2 + b2.  Every product is an fp32 fma chain in ascending k (no split precision, no
// library GEMM).
//   k_kgt_fwd   one workgroup per 32 rows and ALL D columns (D <= kMaxD): the gathered X chunk (32 x 16) and the W1 chunk (16 x D) are
//               staged in LDS (the next chunk is loaded into registers while the current one is multiplied), every thread keeps
//               4 rows x NP column pairs of packed fp32 accumulators (v_pk_fma_f32), the fc2 dot and
//               the optional weighted BCE (main.py:833-840) finish inside the workgroup; the mean loss is the per-workgroup row sums added
//               in block order by the last workgroup to arrive (arrival ticket, release / acquire fences).
//   k_kgt_bwd   dW1 = delta^T X as a split-K product over M: grid (n tile x k tile of 64 x 64, part p of the rows, walked in 64-row
//               chunks whose delta and X slices are staged in LDS, delta made on the fly from z, g_s and w2); each workgroup writes
//               its part's 64 x 64 partial, the last of the P workgroups of a tile to arrive adds the P partials in p order.  The
//               (kb = 0) workgroups also sum db1 = sum delta and dw2 = sum g_s h1 over their rows, the (0, 0) ones db2 = sum g_s: every
//               reduction has one fixed order, so the gradients are bitwise identical from run to run.
#include "recon_common.h"

#pragma clang fp contract(off)

namespace recon {
namespace {

constexpr int kMaxD = 512;                          // documented limit of the scorer entries (RECON_ERR_UNSUPPORTED above)
constexpr int64_t kEntityDrawCap = 1 << 16;
constexpr int kFR = 32, kKC = 16;                   // forward: rows per workgroup, k chunk
constexpr int kBT = 64, kBM = 64, kBP = kBT + 4;    // backward: output tile edge, rows per chunk, LDS row stride
constexpr int kThreads = 256;
constexpr int kBwdTargetBlocks = 1024;              // backward grid: about four workgroups per CU
// Both workspaces start with kTicketWords arrival counters, at the same place whatever (M, D) is: a workspace reused for another shape
// finds them at zero (the last workgroup to arrive resets its counter), while everything after them is rewritten by every call.
constexpr int kTicketWords = 256;
static_assert((kMaxD / kBT) * (3 * kMaxD / kBT) <= kTicketWords, "one arrival counter per backward tile");
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint64_t kgt_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

// uniform id in [0, n) of draw k of row c
__device__ __forceinline__ int64_t kgt_draw(uint64_t seed, uint64_t c, uint64_t k, int64_t n) {
    const uint64_t u = kgt_mix(kgt_mix(kgt_mix(seed) ^ (c * 0x9e3779b97f4a7c15ULL)) ^ (k + 0x632be59bd9b4e019ULL));
    return static_cast<int64_t>(__umul64hi(u, static_cast<uint64_t>(n)));
}

__device__ __forceinline__ bool kgt_known(const int64_t* __restrict__ keys, int64_t nk, int64_t key) {
    int64_t lo = 0, hi = nk;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < nk && keys[lo] == key;
}

__device__ __forceinline__ int64_t kgt_id(const void* tri, int idx64, int64_t m, int col) {
    return idx64 ? static_cast<const int64_t*>(tri)[3 * m + col] : static_cast<int64_t>(static_cast<const int32_t*>(tri)[3 * m + col]);
}

__global__ void __launch_bounds__(kThreads) k_kgt_corrupt(const void* __restrict__ pos, int idx64, const float* __restrict__ vals, int64_t B,
                                                          int32_t r, const int64_t* __restrict__ keys, int64_t nk, int64_t n_ent, int64_t n_rel,
                                                          uint64_t seed, int64_t* __restrict__ out_idx, float* __restrict__ out_val,
                                                          unsigned long long* __restrict__ capped) {
    const int64_t o = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (o >= B * (2 * static_cast<int64_t>(r) + 1)) return;
    const int64_t c = o - B;
    const int64_t b = o < B ? o : c % B;
    int64_t h = kgt_id(pos, idx64, b, 0), rel = kgt_id(pos, idx64, b, 1), t = kgt_id(pos, idx64, b, 2);
    float v = vals[b];
    if (o >= B) {
        const int64_t half = B * (r / 2);
        const int col = c < half ? 0 : c < 2 * half ? 2 : c >= B * r ? 1 : -1;
        if (col == 0 || col == 2) {
            int64_t k = 0;
            for (; k < kEntityDrawCap; ++k) {
                const int64_t id = kgt_draw(seed, static_cast<uint64_t>(c), static_cast<uint64_t>(k), n_ent);
                const int64_t key = col == 0 ? (rel * n_ent + id) * n_ent + t : (rel * n_ent + h) * n_ent + id;
                if (!kgt_known(keys, nk, key)) {
                    if (col == 0) h = id;
                    else t = id;
                    v = -1.f;
                    break;
                }
            }
            if (k == kEntityDrawCap) atomicAdd(capped, 1ULL);
        } else if (col == 1) {
            for (int64_t k = 0; k < n_rel; ++k) {                               // the first draw + n_rel - 1 redraws (:161-170)
                const int64_t id = kgt_draw(seed, static_cast<uint64_t>(c), static_cast<uint64_t>(k), n_rel);
                if (!kgt_known(keys, nk, (id * n_ent + h) * n_ent + t)) {
                    rel = id;
                    v = -1.f;
                    break;
                }
            }
        }
    }
    out_idx[3 * o] = h;
    out_idx[3 * o + 1] = rel;
    out_idx[3 * o + 2] = t;
    out_val[o] = v;
}

struct KgtArgs {
    const void* tri;        // [M][3] int32 or int64
    int32_t idx64;
    int64_t M;
    const float* E;         // [n_ent][D]
    const float* R;         // [n_rel][D]
    int64_t n_ent, n_rel;
    int32_t D;
    float slope;
};

// the ids of row m; false (ids 0) when one lies outside its table
__device__ __forceinline__ bool kgt_row(const KgtArgs& a, int64_t m, int64_t (&id)[3]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        id[j] = kgt_id(a.tri, a.idx64, m, j);
        const int64_t n = j == 1 ? a.n_rel : a.n_ent;
        if (id[j] < 0 || id[j] >= n) { ok = false; id[j] = 0; }
    }
    return ok;
}

// X[m][k] given the row's ids (k < 3 D)
__device__ __forceinline__ float kgt_x(const KgtArgs& a, const int64_t* id, int k) {
    const int seg = (k >= a.D) + (k >= 2 * a.D);
    return (seg == 1 ? a.R : a.E)[id[seg] * a.D + (k - seg * a.D)];
}

struct KgtLoss {            // weighted BCE (main.py:833-840); vals == nullptr: no loss
    const float* vals;      // [M] reference values (+1 / -1)
    float two_r;            // 2 * valid_invalid_ratio_conv
    float* terms;           // [M] weighted per-row term (optional)
    float* g_s;             // [M] dL/ds
    float* loss;            // [1] mean
};

template <int NP>           // column pairs per thread: columns 64 p + 2 tc + {0, 1}, p < NP (D <= 64 NP)
__global__ void __launch_bounds__(kThreads) k_kgt_fwd(const KgtArgs a, const float* __restrict__ W1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ z_out,
                                                      float* __restrict__ s_out, const KgtLoss l, float* __restrict__ part,
                                                      unsigned* __restrict__ ticket) {
    __shared__ float xs[kFR][kKC + 1];
    __shared__ float ws[kKC][NP * 64 + 2];          // W1 chunk transposed; stride = 2 mod 32: the staging writes hit distinct banks
    __shared__ int64_t ids[kFR][3];
    __shared__ int ok[kFR];
    __shared__ float lrow[kFR];
    __shared__ unsigned last;
    const int t = threadIdx.x, tr = t / 32, tc = t % 32;
    const int D = a.D, K = 3 * D;
    const int64_t m0 = static_cast<int64_t>(blockIdx.x) * kFR;
    if (t < kFR) {
        int64_t id[3] = {0, 0, 0};
        ok[t] = m0 + t < a.M && kgt_row(a, m0 + t, id);
        ids[t][0] = id[0]; ids[t][1] = id[1]; ids[t][2] = id[2];
    }
    f32x2 acc[4][NP];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[i][p] = f32x2{0.f, 0.f};
    const int kk_s = t % kKC, r_s = t / kKC;                                // staging: column kk_s of rows / W1 rows r_s + 16 q
    float xr[kFR / 16], wr[NP * 4];                                         // the next chunk, loaded while the current one is multiplied
    __syncthreads();                                                        // ids staged
    auto load = [&](int k0) {
        const int k = k0 + kk_s;
#pragma unroll
        for (int q = 0; q < kFR / 16; ++q) {
            const int row = r_s + 16 * q;
            xr[q] = (k < K && ok[row]) ? kgt_x(a, ids[row], k) : 0.f;
        }
#pragma unroll
        for (int q = 0; q < NP * 4; ++q) {
            const int n = r_s + 16 * q;
            wr[q] = (n < D && k < K) ? W1[static_cast<int64_t>(n) * K + k] : 0.f;
        }
    };
    load(0);
    for (int k0 = 0; k0 < K; k0 += kKC) {
        __syncthreads();                                                    // the previous chunk's readers are done
#pragma unroll
        for (int q = 0; q < kFR / 16; ++q) xs[r_s + 16 * q][kk_s] = xr[q];
#pragma unroll
        for (int q = 0; q < NP * 4; ++q) ws[kk_s][r_s + 16 * q] = wr[q];
        __syncthreads();
        if (k0 + kKC < K) load(k0 + kKC);
        constexpr int kUnrollKK = NP > 6 ? 2 : 4;
#pragma unroll kUnrollKK
        for (int kk = 0; kk < kKC; ++kk) {
            f32x2 w[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) w[p] = *reinterpret_cast<const f32x2*>(&ws[kk][64 * p + 2 * tc]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float x = xs[tr + 8 * i][kk];
                const f32x2 xx = f32x2{x, x};
#pragma unroll
                for (int p = 0; p < NP; ++p) acc[i][p] = __builtin_elementwise_fma(xx, w[p], acc[i][p]);
            }
        }
    }
    const float bias2 = b2[0];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = tr + 8 * i;
        const int64_t m = m0 + row;
        float sp = 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int n = 64 * p + 2 * tc + e;
                if (n < D) {
                    const float zz = acc[i][p][e] + b1[n];
                    if (z_out && m < a.M) z_out[m * D + n] = zz;
                    sp = fmaf(w2[n], fmaxf(zz, zz * a.slope), sp);
                }
            }
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) sp += __shfl_xor(sp, o, 32);
        if (tc == 0) {
            float term = 0.f;
            if (m < a.M) {
                const float s = ok[row] ? sp + bias2 : __builtin_nanf("");
                s_out[m] = s;
                if (l.vals) {
                    const float y = (l.vals[m] + 1.f) / 2.f;
                    const float w = y + (1.f - y) / l.two_r;
                    const float mx = fmaxf(-s, 0.f);
                    term = w * ((1.f - y) * s + mx + logf(expf(-mx) + expf(-s - mx)));
                    if (l.terms) l.terms[m] = term;
                    l.g_s[m] = ((1.f / (1.f + expf(-s)) - y) * w) * (1.f / static_cast<float>(a.M));
                }
            }
            lrow[row] = term;
        }
    }
    if (!l.vals) return;
    __syncthreads();
    if (t == 0) {
        float sum = 0.f;
        for (int row = 0; row < kFR; ++row) sum += lrow[row];
        part[blockIdx.x] = sum;
        __threadfence();                                                    // release the partial
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();                                                        // acquire every workgroup's partial
    if (t < kWave) {                                                        // lane j adds blocks j, j + 64, ... in order, then a fixed tree
        float sum = 0.f;
        for (unsigned blk = t; blk < gridDim.x; blk += kWave) sum += part[blk];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, kWave);
        if (t == 0) {
            l.loss[0] = sum / static_cast<float>(a.M);
            *ticket = 0u;                                                   // ready for the next call
        }
    }
}

struct KgtGrads {
    const float* z;         // [M][D] saved by the forward
    const float* g_s;       // [M]
    const float* g_scale;   // [1] or nullptr: g_s * g_scale
    const float* w2;        // [D]
    float* dW1; float* db1; float* dw2; float* db2;
};

__global__ void __launch_bounds__(kThreads) k_kgt_bwd(const KgtArgs a, const KgtGrads g, int64_t rows_per_part, float* __restrict__ part,
                                                      float* __restrict__ part_vec, unsigned* __restrict__ tickets) {
    __shared__ float dls[kBM][kBP], xs[kBM][kBP];
    __shared__ int64_t rid[kBM][3];
    __shared__ float red[2][4][kBT];
    __shared__ float gsum;
    __shared__ unsigned last;
    const int D = a.D, K = 3 * D;
    const int kt = (K + kBT - 1) / kBT;
    const int P = gridDim.y;
    const int tile = blockIdx.x, nb = tile / kt, kb = tile % kt, p = blockIdx.y;
    const int n0 = nb * kBT, k0 = kb * kBT;
    const int64_t mb = p * rows_per_part, me = mb + rows_per_part < a.M ? mb + rows_per_part : a.M;
    const int t = threadIdx.x, tn = t / 16, tk = t % 16;                    // outputs (n0 + 4 tn + i, k0 + 4 tk + j)
    const int c_s = t % kBT, r_s = t / kBT;                                 // staging: column c_s of rows r_s + 4 q
    const float gscale = g.g_scale ? g.g_scale[0] : 1.f;
    const bool vec = kb == 0;
    f32x2 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = f32x2{0.f, 0.f};
    float db1p = 0.f, dw2p = 0.f;                                           // column n0 + c_s over the rows r_s + 4 q of every chunk
    const int n_s = n0 + c_s;
    const float w2n = n_s < D ? g.w2[n_s] : 0.f;
    for (int64_t mc = mb; mc < me; mc += kBM) {
        __syncthreads();                                                    // the previous chunk's readers are done
        if (t < kBM && mc + t < me) {
            int64_t id[3];
            kgt_row(a, mc + t, id);
            rid[t][0] = id[0]; rid[t][1] = id[1]; rid[t][2] = id[2];
        }
        __syncthreads();
#pragma unroll 4
        for (int q = 0; q < kBM / 4; ++q) {
            const int row = r_s + 4 * q;
            const int64_t m = mc + row;
            float dl = 0.f, x = 0.f;
            if (m < me) {
                if (n_s < D) {
                    const float gm = g.g_s[m] * gscale;
                    const float zz = g.z[m * D + n_s];
                    const float dh = gm * w2n;                              // fc2's backward, then LeakyReLU's (slope at z <= 0)
                    dl = zz > 0.f ? dh : dh * a.slope;
                    if (vec) {
                        db1p += dl;
                        dw2p = fmaf(gm, fmaxf(zz, zz * a.slope), dw2p);
                    }
                }
                const int k = k0 + c_s;
                if (k < K) x = kgt_x(a, rid[row], k);
            }
            dls[row][c_s] = dl;
            xs[row][c_s] = x;
        }
        __syncthreads();
#pragma unroll 8
        for (int mm = 0; mm < kBM; ++mm) {
            const float4 d4 = *reinterpret_cast<const float4*>(&dls[mm][4 * tn]);
            const float4 x4 = *reinterpret_cast<const float4*>(&xs[mm][4 * tk]);
            const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
            const f32x2 xa = f32x2{x4.x, x4.y}, xb = f32x2{x4.z, x4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x2 dd = f32x2{dv[i], dv[i]};
                acc[i][0] = __builtin_elementwise_fma(dd, xa, acc[i][0]);
                acc[i][1] = __builtin_elementwise_fma(dd, xb, acc[i][1]);
            }
        }
    }
    const int64_t DK = static_cast<int64_t>(D) * K;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + 4 * tn + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + 4 * tk + j;
            if (n < D && k < K) part[p * DK + static_cast<int64_t>(n) * K + k] = acc[i][j / 2][j % 2];
        }
    }
    if (vec) {
        red[0][r_s][c_s] = db1p;
        red[1][r_s][c_s] = dw2p;
        if (nb == 0 && t < kWave) {                                         // db2 part: lane j adds rows mb + j, mb + j + 64, ..., then a tree
            float s = 0.f;
            for (int64_t m = mb + t; m < me; m += kWave) s += g.g_s[m] * gscale;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, kWave);
            if (t == 0) gsum = s;
        }
        __syncthreads();
        if (t < kBT && n0 + t < D) {
            part_vec[(static_cast<int64_t>(p) * 2) * D + n0 + t] = ((red[0][0][t] + red[0][1][t]) + red[0][2][t]) + red[0][3][t];
            part_vec[(static_cast<int64_t>(p) * 2 + 1) * D + n0 + t] = ((red[1][0][t] + red[1][1][t]) + red[1][2][t]) + red[1][3][t];
        }
        if (nb == 0 && t == 0) part_vec[static_cast<int64_t>(P) * 2 * D + p] = gsum;
    }
    __threadfence();                                                        // release this part
    __syncthreads();
    if (t == 0) last = atomicAdd(tickets + tile, 1u) == static_cast<unsigned>(P - 1);
    __syncthreads();
    if (!last) return;
    __threadfence();                                                        // acquire the other parts
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + 4 * tn + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + 4 * tk + j;
            if (n < D && k < K) {
                const int64_t off = static_cast<int64_t>(n) * K + k;
                float s = 0.f;
                for (int q = 0; q < P; ++q) s += part[q * DK + off];
                g.dW1[off] = s;
            }
        }
    }
    if (vec && t < kBT && n0 + t < D) {
        float s1 = 0.f, s2 = 0.f;
        for (int q = 0; q < P; ++q) {
            s1 += part_vec[(static_cast<int64_t>(q) * 2) * D + n0 + t];
            s2 += part_vec[(static_cast<int64_t>(q) * 2 + 1) * D + n0 + t];
        }
        g.db1[n0 + t] = s1;
        g.dw2[n0 + t] = s2;
    }
    if (vec && nb == 0 && t == 0) {
        float s = 0.f;
        for (int q = 0; q < P; ++q) s += part_vec[static_cast<int64_t>(P) * 2 * D + q];
        g.db2[0] = s;
    }
    if (t == 0) tickets[tile] = 0u;                                         // ready for the next call
}

int kgt_args(KgtArgs& a, const void* tri, int32_t index_bytes, int64_t M, const float* E, const float* R, int64_t n_ent, int64_t n_rel, int32_t D,
             float slope) {
    if (M < 0 || D < 1 || n_ent < 1 || n_rel < 1 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (D > kMaxD || M > 0x7fffffffLL) return RECON_ERR_UNSUPPORTED;
    if (!(slope >= 0.f && slope <= 1.f)) return RECON_ERR_UNSUPPORTED;     // leaky(x) = max(x, slope x) holds on [0, 1]
    if (!tri || !E || !R) return RECON_ERR_INVALID;
    a.tri = tri; a.idx64 = index_bytes == 8; a.M = M;
    a.E = E; a.R = R; a.n_ent = n_ent; a.n_rel = n_rel; a.D = D; a.slope = slope;
    return RECON_OK;
}

// backward split: P parts of rows_per_part rows (a multiple of kBM), a function of (M, D) only
void kgt_bwd_split(int64_t M, int32_t D, int64_t& tiles, int64_t& P, int64_t& rows_per_part) {
    tiles = ceil_div64(D, kBT) * ceil_div64(3 * static_cast<int64_t>(D), kBT);
    P = ceil_div64(kBwdTargetBlocks, tiles);
    const int64_t max_p = ceil_div64(M > 0 ? M : 1, kBM);
    if (P > max_p) P = max_p;
    rows_per_part = ceil_div64(ceil_div64(M > 0 ? M : 1, P), kBM) * kBM;
    P = ceil_div64(M > 0 ? M : 1, rows_per_part);
}

}  // namespace
}  // namespace recon

extern "C" int recon_kg_corrupt(const void* positives, int32_t index_bytes, const float* values, int64_t B, int32_t ratio, const int64_t* keys,
                                int64_t n_keys, int64_t n_ent, int64_t n_rel, uint64_t seed, int64_t* indices, float* out_values,
                                unsigned long long* capped, recon_stream_t stream) {
    if (B < 0 || ratio < 0 || n_keys < 0 || n_ent < 1 || n_rel < 1 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (n_ent > (int64_t{1} << 31) || n_rel > (int64_t{1} << 31) || n_rel > (int64_t{1} << 62) / n_ent / n_ent) return RECON_ERR_UNSUPPORTED;
    if (B * (2 * static_cast<int64_t>(ratio) + 1) > 0x7fffffffLL * recon::kThreads) return RECON_ERR_UNSUPPORTED;
    if (B == 0) return RECON_OK;
    if (!positives || !values || !indices || !out_values || !capped || (n_keys > 0 && !keys)) return RECON_ERR_INVALID;
    const int64_t rows = B * (2 * static_cast<int64_t>(ratio) + 1);
    hipLaunchKernelGGL(recon::k_kgt_corrupt, dim3(static_cast<unsigned>(ceil_div64(rows, recon::kThreads))), dim3(recon::kThreads), 0,
                       as_stream(stream), positives, index_bytes == 8, values, B, ratio, keys, n_keys, n_ent, n_rel, seed, indices, out_values,
                       capped);
    return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
}

extern "C" size_t recon_convkb_train_fwd_workspace_floats(int64_t M, int32_t D) {
    (void)D;
    return M > 0 ? static_cast<size_t>(recon::kTicketWords + ceil_div64(M, recon::kFR)) : 0;
}

extern "C" int recon_convkb_train_fwd(const void* triples, int32_t index_bytes, int64_t M, const float* E, const float* Rel, int64_t n_ent,
                                      int64_t n_rel, int32_t D, const float* W1, const float* b1, const float* w2, const float* b2, float slope,
                                      float* z, float* scores, const float* values, int32_t ratio, float* loss_terms, float* g_scores, float* loss,
                                      float* workspace, size_t workspace_floats, recon_stream_t stream) {
    recon::KgtArgs a;
    const int st = recon::kgt_args(a, triples, index_bytes, M, E, Rel, n_ent, n_rel, D, slope);
    if (st != RECON_OK) return st;
    if (!W1 || !b1 || !w2 || !b2 || !scores) return RECON_ERR_INVALID;
    recon::KgtLoss l{values, 2.f * static_cast<float>(ratio), loss_terms, g_scores, loss};
    if (values && (ratio < 1 || !g_scores || !loss)) return RECON_ERR_INVALID;   // the weights divide by 2 r (main.py:838)
    if (M == 0) return RECON_OK;
    const int64_t blocks = ceil_div64(M, recon::kFR);
    if (values && (!workspace || workspace_floats < recon_convkb_train_fwd_workspace_floats(M, D))) return RECON_ERR_WORKSPACE;
    unsigned* ticket = values ? reinterpret_cast<unsigned*>(workspace) : nullptr;
    float* part = values ? workspace + recon::kTicketWords : nullptr;
    const dim3 grid(static_cast<unsigned>(blocks)), block(recon::kThreads);
    hipStream_t s = as_stream(stream);
    switch ((D + 63) / 64) {
#define KGT_FWD(NP) \
    case NP: hipLaunchKernelGGL(recon::k_kgt_fwd<NP>, grid, block, 0, s, a, W1, b1, w2, b2, z, scores, l, part, ticket); break;
        KGT_FWD(1) KGT_FWD(2) KGT_FWD(3) KGT_FWD(4) KGT_FWD(5) KGT_FWD(6) KGT_FWD(7) KGT_FWD(8)
#undef KGT_FWD
        default: return RECON_ERR_UNSUPPORTED;
    }
    return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
}

extern "C" size_t recon_convkb_train_bwd_workspace_floats(int64_t M, int32_t D) {
    if (M <= 0 || D <= 0) return 0;
    int64_t tiles, P, rpp;
    recon::kgt_bwd_split(M, D, tiles, P, rpp);
    return static_cast<size_t>(recon::kTicketWords + P * D * 3 * static_cast<int64_t>(D) + P * 2 * D + P);
}

extern "C" int recon_convkb_train_bwd(const void* triples, int32_t index_bytes, int64_t M, const float* E, const float* Rel, int64_t n_ent,
                                      int64_t n_rel, int32_t D, const float* w2, float slope, const float* z, const float* g_scores,
                                      const float* g_scale, float* dW1, float* db1, float* dw2, float* db2, float* workspace,
                                      size_t workspace_floats, recon_stream_t stream) {
    recon::KgtArgs a;
    const int st = recon::kgt_args(a, triples, index_bytes, M, E, Rel, n_ent, n_rel, D, slope);
    if (st != RECON_OK) return st;
    if (!w2 || !dW1 || !db1 || !dw2 || !db2) return RECON_ERR_INVALID;
    hipStream_t s = as_stream(stream);
    if (M == 0) {                                                           // empty sums
        if (hipMemsetAsync(dW1, 0, sizeof(float) * 3 * static_cast<size_t>(D) * D, s) != hipSuccess ||
            hipMemsetAsync(db1, 0, sizeof(float) * D, s) != hipSuccess || hipMemsetAsync(dw2, 0, sizeof(float) * D, s) != hipSuccess ||
            hipMemsetAsync(db2, 0, sizeof(float), s) != hipSuccess)
            return RECON_ERR_LAUNCH;
        return RECON_OK;
    }
    if (!z || !g_scores) return RECON_ERR_INVALID;
    if (!workspace || workspace_floats < recon_convkb_train_bwd_workspace_floats(M, D)) return RECON_ERR_WORKSPACE;
    int64_t tiles, P, rpp;
    recon::kgt_bwd_split(M, D, tiles, P, rpp);
    unsigned* tickets = reinterpret_cast<unsigned*>(workspace);
    float* part = workspace + recon::kTicketWords;
    float* part_vec = part + P * D * 3 * static_cast<int64_t>(D);
    recon::KgtGrads g{z, g_scores, g_scale, w2, dW1, db1, dw2, db2};
    hipLaunchKernelGGL(recon::k_kgt_bwd, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(P)), dim3(recon::kThreads), 0, s, a, g, rpp, part,
                       part_vec, tickets);
    return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
}
