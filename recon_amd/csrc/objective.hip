// E13 — the stage-B objective between the logits and the optimiser (train.py:232, :309-324, test.py:274-291,
// utils/evaluation_utils.py:17-59): CrossEntropyLoss(ignore_index) over [M][n_out], torch.max's indices, the softmax probability of the
// prediction and the three counters of evaluate_instance_based, without the [M][n_out] log-softmax and without a host read:
//     ls[m]   = log sum_c exp(x[m][c] - max_m)                            term[m] = ls[m] - (x[m][label[m]] - max_m)
//     loss    = (sum over kept m, ascending, of term[m]) / kept           kept: label[m] != ignore_index
//     pred[m] = lowest index of the row's maximum, a NaN counting as the maximum          conf[m] = 1 / sum_c exp(x[m][c] - max_m)
//     counts  = {kept, kept & pred != empty, kept & label != empty, kept & pred == label != empty}
//     prec = n_ok / n_pred (0 at n_pred == 0), rec = n_ok / n_gold (0 at n_gold == 0), f1 = 2.0 prec rec / (prec + rec) (0 at prec + rec == 0)
// A kept row whose label lies outside [0, n_out) has the term NaN and a zero gradient row; its label is never used as an address.
// +inf, -inf and NaN go through the plain arithmetic above, which is log_softmax's.  No atomics, every sum in an order M and n_out decide.
//
// k_ro_rows: a wavefront per row, four rows per workgroup.  The split: a row of n_out <= 512 = 64 lanes x 8 values is read ONCE into
//   NV = 1, 2, 4, 6 or 8 registers per lane (value j of a lane is column lane + 64 j: coalesced; n_out = 353, the reference's width, is
//   NV = 6 with a tail of 33) and the maximum, its index and the exp-sum are taken from the registers; a wider row (513 .. 8192) is walked
//   twice, once for the maximum and its index, once for the exp-sum.  The maximum and its index travel as ONE 64-bit key (the value's
//   order-preserving bits, all ones for a NaN, above the complement of the index), so a butterfly of six maxima leaves the winner in
//   every lane; the exp-sum is group_sum<64>.  Lane 0 writes the row's term, ls (when asked), prediction and confidence.  ls, the
//   log-sum-exp LESS the maximum, is the float per row the backward keeps: with the maximum added in fp32 the softmax would carry the
//   maximum's rounding (half an ulp of 12 is 5e-7 of every probability); the maximum itself is exact and the backward takes it again.
// k_ro_combine: ONE workgroup; thread t adds the terms of the kept rows t, t + 256, ... upwards in fp64 and counts, the 256 partial sums
//   are added by a fixed tree, thread 0 rounds the loss once to fp32, forms the fp64 F1 and adds to the accumulator's buffers when given
//   them (plain read-modify-write: calls on one stream are ordered).  A launch of its own: loss.hip's k_transe_mean records what the
//   "last workgroup reduces" form cost there (a device-scope fence per workgroup, 208 us for 10 us of work).
// k_ro_bwd: a wavefront per row, the same split; d_logits[m][c] = g (exp((x[m][c] - max_m) - ls[m]) - [c == label[m]]) / kept for a kept
//   row with a label inside [0, n_out), zero otherwise and when kept == 0; g and kept are read from device memory.  Every cell is
//   written exactly once.
#include "recon_common.h"

#include <cmath>

namespace recon {
namespace {

constexpr int kRoThreads = 256;
constexpr int kRoRows = kRoThreads / kWave;          // rows per workgroup
constexpr int kRoRegWidth = 8 * kWave;               // the widest row held in registers
constexpr int kRoMaxWidth = 8192;
constexpr int64_t kRoMaxRows = int64_t{1} << 30;

// order-preserving bits of a float, all ones for a NaN; -0 counts as +0 (torch.max: an exact tie)
__device__ __forceinline__ uint32_t ro_order(float v) {
    if (v != v) return 0xffffffffu;
    if (v == 0.f) v = 0.f;
    const uint32_t b = __builtin_bit_cast(uint32_t, v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ro_value(uint32_t k) {
    if (k == 0xffffffffu) return __builtin_nanf("");
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// (value, column) as one key: the larger value wins, the lower column among equal values.  Every real cell's key is above 0.
__device__ __forceinline__ uint64_t ro_key(float v, int c) {
    return (static_cast<uint64_t>(ro_order(v)) << 32) | static_cast<uint32_t>(0x7fffffff - c);
}
__device__ __forceinline__ uint64_t ro_wave_max(uint64_t k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t hi = __shfl_xor(static_cast<uint32_t>(k >> 32), off, kWave), lo = __shfl_xor(static_cast<uint32_t>(k), off, kWave);
        const uint64_t o = (static_cast<uint64_t>(hi) << 32) | lo;
        k = o > k ? o : k;
    }
    return k;
}

__device__ __forceinline__ uint32_t ro_wave_max32(uint32_t k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(k, off, kWave);
        k = o > k ? o : k;
    }
    return k;
}

// NV > 0: the row in NV registers per lane; NV == 0: two walks over the row
template <int NV>
__global__ void __launch_bounds__(kRoThreads) k_ro_rows(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels, int64_t M,
                                                        int32_t n, int64_t ignore_index, float* __restrict__ terms, float* __restrict__ lse_out,
                                                        int64_t* __restrict__ predicted, float* __restrict__ confidence) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t m = static_cast<int64_t>(blockIdx.x) * kRoRows + (threadIdx.x >> 6);
    if (m >= M) return;                                                  // (wave-uniform)
    const float* x = logits + m * ld;
    uint64_t key = 0;
    float s = 0.f, mx;
    if constexpr (NV > 0) {
        float v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = lane + kWave * j;
            v[j] = c < n ? x[c] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = lane + kWave * j;
            const uint64_t k = c < n ? ro_key(v[j], c) : 0;
            key = k > key ? k : key;
        }
        key = ro_wave_max(key);
        mx = ro_value(static_cast<uint32_t>(key >> 32));
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = lane + kWave * j;
            s += c < n ? expf(v[j] - mx) : 0.f;
        }
    } else {
        for (int c = lane; c < n; c += kWave) {
            const uint64_t k = ro_key(x[c], c);
            key = k > key ? k : key;
        }
        key = ro_wave_max(key);
        mx = ro_value(static_cast<uint32_t>(key >> 32));
        for (int c = lane; c < n; c += kWave) s += expf(x[c] - mx);
    }
    s = group_sum<64>(s);
    if (lane == 0) {
        const float ls = logf(s);
        predicted[m] = 0x7fffffff - static_cast<int64_t>(static_cast<uint32_t>(key));
        confidence[m] = 1.f / s;
        if (lse_out) lse_out[m] = ls;
        if (terms) {
            const int64_t lab = labels[m];
            float t = 0.f;                                               // an ignored row's term is never read
            if (lab != ignore_index) t = (lab >= 0 && lab < n) ? ls - (x[lab] - mx) : __builtin_nanf("");
            terms[m] = t;
        }
    }
}

__global__ void __launch_bounds__(kRoThreads) k_ro_combine(const float* __restrict__ terms, const int64_t* __restrict__ labels,
                                                           const int64_t* __restrict__ predicted, int64_t M, int64_t ignore_index,
                                                           int64_t empty_label, float* __restrict__ loss, int64_t* __restrict__ counts,
                                                           double* __restrict__ f1_out, int64_t* __restrict__ acc_counts,
                                                           double* __restrict__ acc_f1_sum, int64_t* __restrict__ acc_batches) {
    __shared__ double red[kRoThreads];
    __shared__ int cnt[4][kRoThreads];
    const int t = threadIdx.x;
    double s = 0.0;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int64_t m = t; m < M; m += kRoThreads) {                        // thread t: rows t, t + 256, ... in order
        const int64_t lab = labels[m], p = predicted[m];
        if (lab == ignore_index) continue;
        s += static_cast<double>(terms[m]);
        c0 += 1;
        c1 += p != empty_label;
        c2 += lab != empty_label;
        c3 += lab != empty_label && p == lab;
    }
    red[t] = s;
    cnt[0][t] = c0;
    cnt[1][t] = c1;
    cnt[2][t] = c2;
    cnt[3][t] = c3;
    __syncthreads();
    for (int off = kRoThreads / 2; off > 0; off >>= 1) {
        if (t < off) {
            red[t] += red[t + off];
#pragma unroll
            for (int q = 0; q < 4; ++q) cnt[q][t] += cnt[q][t + off];
        }
        __syncthreads();
    }
    if (t == 0) {
        const int64_t kept = cnt[0][0], n_pred = cnt[1][0], n_gold = cnt[2][0], n_ok = cnt[3][0];
        loss[0] = static_cast<float>(red[0] / static_cast<double>(kept));       // kept == 0: 0 / 0 = NaN, what the stock line gives
        const double prec = n_pred > 0 ? static_cast<double>(n_ok) / static_cast<double>(n_pred) : 0.0;
        const double rec = n_gold > 0 ? static_cast<double>(n_ok) / static_cast<double>(n_gold) : 0.0;
        const double f1 = (rec + prec) > 0.0 ? 2.0 * prec * rec / (prec + rec) : 0.0;
        counts[0] = kept;
        counts[1] = n_pred;
        counts[2] = n_gold;
        counts[3] = n_ok;
        f1_out[0] = f1;
        if (acc_counts) {
            acc_counts[0] += kept;
            acc_counts[1] += n_pred;
            acc_counts[2] += n_gold;
            acc_counts[3] += n_ok;
            acc_f1_sum[0] += f1;
            acc_batches[0] += 1;
        }
    }
}

template <int NV>
__global__ void __launch_bounds__(kRoThreads) k_ro_bwd(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                       const float* __restrict__ lse, const float* __restrict__ g_loss,
                                                       const int64_t* __restrict__ counts, int64_t M, int32_t n, int64_t ignore_index,
                                                       float* __restrict__ g_logits) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t m = static_cast<int64_t>(blockIdx.x) * kRoRows + (threadIdx.x >> 6);
    if (m >= M) return;
    const int64_t kept = counts[0], lab = labels[m];
    float* g = g_logits + m * n;
    if (kept <= 0 || lab == ignore_index || lab < 0 || lab >= n) {       // (wave-uniform)
        for (int c = lane; c < n; c += kWave) g[c] = 0.f;
        return;
    }
    const float* x = logits + m * ld;
    const float scale = g_loss[0] / static_cast<float>(kept), ls = lse[m];
    const int at = static_cast<int>(lab);
    uint32_t key = 0;
    if constexpr (NV > 0) {
        float v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = lane + kWave * j;
            v[j] = c < n ? x[c] : 0.f;
            const uint32_t k = c < n ? ro_order(v[j]) : 0u;
            key = k > key ? k : key;
        }
        const float mx = ro_value(ro_wave_max32(key));
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = lane + kWave * j;
            if (c < n) g[c] = scale * (expf((v[j] - mx) - ls) - (c == at ? 1.f : 0.f));
        }
    } else {
        for (int c = lane; c < n; c += kWave) {
            const uint32_t k = ro_order(x[c]);
            key = k > key ? k : key;
        }
        const float mx = ro_value(ro_wave_max32(key));
        for (int c = lane; c < n; c += kWave) g[c] = scale * (expf((x[c] - mx) - ls) - (c == at ? 1.f : 0.f));
    }
}

bool ro_shape_ok(int64_t M, int32_t n) { return M >= 0 && M <= kRoMaxRows && n >= 1 && n <= kRoMaxWidth; }

// fn<NV> for the registers per lane a width takes (0: the two walks)
#define RO_BY_WIDTH(n_out, call)                              \
    do {                                                      \
        if ((n_out) <= kWave) { call(1); }                    \
        else if ((n_out) <= 2 * kWave) { call(2); }           \
        else if ((n_out) <= 4 * kWave) { call(4); }           \
        else if ((n_out) <= 6 * kWave) { call(6); }           \
        else if ((n_out) <= kRoRegWidth) { call(8); }         \
        else { call(0); }                                     \
    } while (0)

template <int NV>
void ro_launch_rows(hipStream_t st, const float* logits, int64_t ld, const int64_t* labels, int64_t M, int32_t n, int64_t ignore_index, float* terms,
                    float* lse, int64_t* predicted, float* confidence) {
    hipLaunchKernelGGL(k_ro_rows<NV>, dim3(static_cast<unsigned>(ceil_div64(M, kRoRows))), dim3(kRoThreads), 0, st, logits, ld, labels, M, n,
                       ignore_index, terms, lse, predicted, confidence);
}

}  // namespace
}  // namespace recon

extern "C" int recon_relation_objective_supported(int64_t M, int32_t n_out) { return recon::ro_shape_ok(M, n_out) ? 1 : 0; }

extern "C" size_t recon_relation_objective_workspace_bytes(int64_t M, int32_t n_out) {
    if (!recon::ro_shape_ok(M, n_out) || M == 0) return 0;
    return align_up(static_cast<size_t>(M) * sizeof(float), 16);
}

extern "C" int recon_relation_objective_fwd(const float* logits, int64_t ld, const int64_t* labels, int64_t M, int32_t n_out, int64_t ignore_index,
                                            int64_t empty_label, float* loss, int64_t* predicted, float* confidence, float* lse, int64_t* counts,
                                            double* f1, int64_t* acc_counts, double* acc_f1_sum, int64_t* acc_batches, void* workspace,
                                            size_t workspace_bytes, recon_stream_t stream) {
    using namespace recon;
    if (M < 0 || n_out < 1) return RECON_ERR_INVALID;
    if (!ro_shape_ok(M, n_out)) return RECON_ERR_UNSUPPORTED;
    if (M == 0) return RECON_OK;
    if (!logits || !predicted || !confidence || ld < n_out) return RECON_ERR_INVALID;
    const bool acc = acc_counts || acc_f1_sum || acc_batches;
    if (labels) {
        if (!loss || !counts || !f1 || (acc && !(acc_counts && acc_f1_sum && acc_batches))) return RECON_ERR_INVALID;
        if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return RECON_ERR_INVALID;
        if (workspace_bytes < recon_relation_objective_workspace_bytes(M, n_out)) return RECON_ERR_WORKSPACE;
    } else if (loss || counts || f1 || lse || acc) {
        return RECON_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    float* terms = labels ? static_cast<float*>(workspace) : nullptr;
#define RO_ROWS(NV) ro_launch_rows<NV>(st, logits, ld, labels, M, n_out, ignore_index, terms, lse, predicted, confidence)
    RO_BY_WIDTH(n_out, RO_ROWS);
#undef RO_ROWS
    RECON_CHECK_LAUNCH();
    if (labels) {
        hipLaunchKernelGGL(k_ro_combine, dim3(1), dim3(kRoThreads), 0, st, terms, labels, predicted, M, ignore_index, empty_label, loss, counts, f1,
                           acc_counts, acc_f1_sum, acc_batches);
        RECON_CHECK_LAUNCH();
    }
    return RECON_OK;
}

extern "C" int recon_relation_objective_bwd(const float* logits, int64_t ld, const int64_t* labels, const float* lse, const float* g_loss,
                                            const int64_t* counts, int64_t M, int32_t n_out, int64_t ignore_index, float* g_logits,
                                            recon_stream_t stream) {
    using namespace recon;
    if (M < 0 || n_out < 1) return RECON_ERR_INVALID;
    if (!ro_shape_ok(M, n_out)) return RECON_ERR_UNSUPPORTED;
    if (M == 0) return RECON_OK;
    if (!logits || !labels || !lse || !g_loss || !counts || !g_logits || ld < n_out) return RECON_ERR_INVALID;
    hipStream_t st = as_stream(stream);
#define RO_BWD(NV)                                                                                                                        \
    hipLaunchKernelGGL(k_ro_bwd<NV>, dim3(static_cast<unsigned>(ceil_div64(M, kRoRows))), dim3(kRoThreads), 0, st, logits, ld, labels, lse, \
                       g_loss, counts, M, n_out, ignore_index, g_logits)
    RO_BY_WIDTH(n_out, RO_BWD);
#undef RO_BWD
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}
