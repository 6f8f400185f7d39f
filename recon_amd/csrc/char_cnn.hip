// The entity-context encoder's character CNN (models/models.py:57-61) as one device op:
//     pre[s][t][o] = bias[o] + sum_k sum_c E[chars[s][t + k]][c] W[o][c][k]
//     out[s][w][o] = tanh(max over t in [w span, (w + 1) span) of pre[s][t][o]),      chars [S][cfs - 1 + W span], out [S][W][Fo].
// The reference (and the op chain this replaces) writes the gathered embedding [S][Lc][C], its permutation, the convolution and the pool;
// here nothing of size S Lc exists.  Without dropout the convolution of an embedding collapses into table lookups:
//     pre[s][t][o] = bias[o] + sum_k T[k][chars[s][t + k]][o],      T[k] = E . W[:, :, k]^T      (cfs tables of V x Fo).
//
// k_char_tables: T[k][v][o], one thread per element, c ascending.
// k_char_table_fwd: 4 waves per workgroup, ONE WAVE PER WORD, lane = output channel o (Fo > 64: passes of 64).  The span + cfs - 1 ids
//   of the word are read once (lane j holds id j) and handed round with v_readlane: the table row is wave-uniform, the lanes read Fo
//   consecutive floats of it — conflict-free at every row pitch, so the tables lie in LDS unpadded ([cfs][V][Fo], 54 KB at the
//   reference's sizes) while they fit and are read through L2 when they do not (same code, other pointer).  The first maximum of the
//   window wins, as torch's pool picks it; its position goes out as one byte per (s, w, o) beside tanh(max).
// k_char_table_bwd: d_pre = g_out (1 - out^2) goes to dT[k][chars[t* + k]][o] and d_bias[o].  No floating-point atomics: workgroup g owns
//   a fixed run of words and a private dT (LDS while it fits, else its slab of the workspace, zeroed by the host call); inside the
//   workgroup wave j owns the taps k = j, j + 4, ... and lane l the channels o = l mod 64, so every cell has ONE writer that walks the
//   words in order.  k_char_reduce adds the slabs in workgroup order; k_char_param_grads forms dE = sum_k dT[k] . W[:, :, k] (padding row
//   zero) and dW[:, :, k] = dT[k]^T . E.  Every sum has one order: bitwise identical from run to run.
#include <math.h>
#include "ctx_enc_common.h"

namespace recon {
namespace {

constexpr int kCcMaxFo = 256;                 // 4 passes of 64 channels
constexpr int kCcMaxTaps = 16;
constexpr int kCcLdsBytes = 144 * 1024;       // tables / private dT up to this size live in LDS
constexpr int kCcBwdBatch = 8;                // words whose loads are in flight together in the backward
constexpr int64_t kCcMaxTable = 1 << 22;      // cfs V Fo floats

__global__ void __launch_bounds__(256) k_char_tables(const float* __restrict__ E, const float* __restrict__ Wc, int32_t cfs, int32_t V, int32_t C,
                                                     int32_t Fo, float* __restrict__ T) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= static_cast<int64_t>(cfs) * V * Fo) return;
    const int o = static_cast<int>(i % Fo), v = static_cast<int>((i / Fo) % V), k = static_cast<int>(i / (static_cast<int64_t>(Fo) * V));
    const float* e = E + static_cast<int64_t>(v) * C;
    const float* w = Wc + static_cast<int64_t>(o) * C * cfs + k;
    float acc = 0.f;
    for (int c = 0; c < C; ++c) acc = fmaf(e[c], w[static_cast<int64_t>(c) * cfs], acc);
    T[i] = acc;
}

template <bool LDS, typename IdT>
__global__ void __launch_bounds__(256) k_char_table_fwd(const IdT* __restrict__ chars, int64_t ld_chars, const float* __restrict__ T,
                                                        const float* __restrict__ bias, int64_t n_words, int32_t W, int32_t span, int32_t cfs,
                                                        int32_t V, int32_t Fo, float* __restrict__ out, uint8_t* __restrict__ arg) {
    extern __shared__ float cc_lds[];
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const float* tab = T;
    if constexpr (LDS) {
        const int n = cfs * V * Fo;
        for (int i = t; i < n; i += 256) cc_lds[i] = T[i];
        __syncthreads();
        tab = cc_lds;
    }
    const int n_ids = span + cfs - 1;
    const int64_t n_waves = static_cast<int64_t>(gridDim.x) * 4;
    for (int64_t word = static_cast<int64_t>(blockIdx.x) * 4 + wid; word < n_words; word += n_waves) {
        const int64_t s = word / W;
        const int w = static_cast<int>(word - s * W);
        const int idv = word_ids(chars + s * ld_chars + static_cast<int64_t>(w) * span, lane, n_ids, V);
        for (int ob = 0; ob < Fo; ob += 64) {
            const bool live = ob + lane < Fo;
            const int o = live ? ob + lane : Fo - 1;
            const float b = bias[o];
            float best = 0.f;
            int best_t = 0;
            for (int p = 0; p < span; ++p) {
                float pre = b;
                for (int k = 0; k < cfs; ++k) {
                    const int id = __builtin_amdgcn_readlane(idv, p + k);
                    pre += tab[(k * V + id) * Fo + o];
                }
                if (p == 0 || pre > best) { best = pre; best_t = p; }
            }
            if (live) {
                const int64_t at = word * Fo + o;
                out[at] = tanhf(best);
                if (arg) arg[at] = static_cast<uint8_t>(best_t);
            }
        }
    }
}

template <bool LDS, typename IdT>
__global__ void __launch_bounds__(256) k_char_table_bwd(const IdT* __restrict__ chars, int64_t ld_chars, const float* __restrict__ g_out,
                                                        const float* __restrict__ out, const uint8_t* __restrict__ arg, int64_t n_words,
                                                        int64_t words_per_wg, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t Fo,
                                                        float* __restrict__ partial) {
    extern __shared__ float cc_lds[];
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6, n_waves = blockDim.x >> 6;
    const int n = cfs * V * Fo;
    float* slab = partial + static_cast<int64_t>(blockIdx.x) * (n + Fo);       // [cfs][V][Fo] then d_bias [Fo]
    float* acc = slab;
    if constexpr (LDS) {
        for (int i = t; i < n; i += blockDim.x) cc_lds[i] = 0.f;
        __syncthreads();
        acc = cc_lds;
    }
    const int n_ids = span + cfs - 1;
    const int64_t w0 = static_cast<int64_t>(blockIdx.x) * words_per_wg, w1 = min64(w0 + words_per_wg, n_words);
    for (int ob = 0; ob < Fo; ob += 64) {
        const bool live = ob + lane < Fo;
        const int o = live ? ob + lane : Fo - 1;
        float db = 0.f;
        for (int64_t wb = w0; wb < w1; wb += kCcBwdBatch) {
            float d[kCcBwdBatch];
            int ts[kCcBwdBatch], idv[kCcBwdBatch];
#pragma unroll
            for (int u = 0; u < kCcBwdBatch; ++u) {                       // every load of the batch is issued before the first use
                const int64_t word = min64(wb + u, w1 - 1);
                const int64_t s = word / W;
                const int w = static_cast<int>(word - s * W);
                idv[u] = word_ids(chars + s * ld_chars + static_cast<int64_t>(w) * span, lane, n_ids, V);
                const int64_t at = word * Fo + o;
                const float y = out[at];
                d[u] = (live && wb + u < w1) ? g_out[at] * (1.f - y * y) : 0.f;
                ts[u] = min(static_cast<int>(arg[at]), span - 1);
            }
#pragma unroll
            for (int u = 0; u < kCcBwdBatch; ++u) {
                if (wid == 0) db += d[u];
                for (int k = wid; k < cfs; k += n_waves) {
                    const int id = __shfl(idv[u], ts[u] + k, 64);
                    if (live && wb + u < w1) acc[(k * V + id) * Fo + o] += d[u];
                }
            }
        }
        if (wid == 0 && live) slab[n + o] = db;
    }
    if constexpr (LDS) {
        __syncthreads();
        for (int i = t; i < n; i += blockDim.x) slab[i] = cc_lds[i];
    }
}

// total[i] = sum over the G slabs, in slab order; the first n elements are dT, the last Fo d_bias
__global__ void __launch_bounds__(256) k_char_reduce(const float* __restrict__ partial, int32_t G, int32_t n, int32_t Fo, float* __restrict__ dT,
                                                     float* __restrict__ g_bias) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n + Fo) return;
    const int64_t slab = static_cast<int64_t>(n) + Fo;
    float sum = 0.f;
#pragma unroll 8
    for (int g = 0; g < G; ++g) sum += partial[g * slab + i];
    if (i < n) dT[i] = sum; else g_bias[i - n] = sum;
}

// threads [0, V C): g_emb[v][c] = sum_k sum_o dT[k][v][o] W[o][c][k] (row padding_idx: 0);  then [0, Fo C cfs): g_w[o][c][k] = sum_v dT[k][v][o] E[v][c]
__global__ void __launch_bounds__(256) k_char_param_grads(const float* __restrict__ dT, const float* __restrict__ E, const float* __restrict__ Wc,
                                                          int32_t cfs, int32_t V, int32_t C, int32_t Fo, int32_t padding_idx,
                                                          float* __restrict__ g_emb, float* __restrict__ g_w) {
    int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int64_t n_emb = static_cast<int64_t>(V) * C, n_w = static_cast<int64_t>(Fo) * C * cfs;
    if (i < n_emb) {
        const int c = static_cast<int>(i % C), v = static_cast<int>(i / C);
        float acc = 0.f;
        if (v != padding_idx) {
            for (int k = 0; k < cfs; ++k) {
                const float* dt = dT + (static_cast<int64_t>(k) * V + v) * Fo;
                for (int o = 0; o < Fo; ++o) acc = fmaf(dt[o], Wc[(static_cast<int64_t>(o) * C + c) * cfs + k], acc);
            }
        }
        g_emb[i] = acc;
        return;
    }
    i -= n_emb;
    if (i >= n_w) return;
    const int k = static_cast<int>(i % cfs), c = static_cast<int>((i / cfs) % C), o = static_cast<int>(i / (static_cast<int64_t>(cfs) * C));
    const float* dt = dT + static_cast<int64_t>(k) * V * Fo + o;
    float acc = 0.f;
    for (int v = 0; v < V; ++v) acc = fmaf(dt[static_cast<int64_t>(v) * Fo], E[static_cast<int64_t>(v) * C + c], acc);
    g_w[i] = acc;
}

inline int64_t cc_table_floats(int32_t cfs, int32_t V, int32_t Fo) { return static_cast<int64_t>(cfs) * V * Fo; }

// workgroups of the backward and the words each owns
inline void cc_bwd_split(int64_t n_words, int64_t table_bytes, int64_t* words_per_wg, int32_t* G) {
    const int64_t max_wg = 2 * table_bytes <= 160 * 1024 ? 512 : 256;    // two workgroups per CU while two private dT fit in its LDS
    split_rows(n_words, max_wg, 2 * kCcBwdBatch, words_per_wg, G);
}

template <bool LDS, typename IdT>
int cc_launch_fwd(const void* chars, int64_t ld_chars, const float* T, const float* bias, int64_t n_words, int32_t W, int32_t span, int32_t cfs,
                  int32_t V, int32_t Fo, float* out, uint8_t* arg, hipStream_t st) {
    const size_t lds = LDS ? static_cast<size_t>(cc_table_floats(cfs, V, Fo)) * 4 : 0;
    auto kern = &k_char_table_fwd<LDS, IdT>;
    if (!allow_lds(kern, lds)) return RECON_ERR_LAUNCH;
    const int64_t blocks = LDS ? min64(ceil_div64(n_words, 32), 512) : min64(ceil_div64(n_words, 4), 4096);
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks)), dim3(256), lds, st, static_cast<const IdT*>(chars), ld_chars, T, bias, n_words, W,
                       span, cfs, V, Fo, out, arg);
    return RECON_OK;
}

template <bool LDS, typename IdT>
int cc_launch_bwd(const void* chars, int64_t ld_chars, const float* g_out, const float* out, const uint8_t* arg, int64_t n_words,
                  int64_t words_per_wg, int32_t G, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t Fo, float* partial, hipStream_t st) {
    const size_t lds = LDS ? static_cast<size_t>(cc_table_floats(cfs, V, Fo)) * 4 : 0;
    auto kern = &k_char_table_bwd<LDS, IdT>;
    if (!allow_lds(kern, lds)) return RECON_ERR_LAUNCH;
    const int waves = cfs < 4 ? cfs : 4;
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(G)), dim3(64 * waves), lds, st, static_cast<const IdT*>(chars), ld_chars, g_out, out, arg,
                       n_words, words_per_wg, W, span, cfs, V, Fo, partial);
    return RECON_OK;
}

}  // namespace
}  // namespace recon

extern "C" int recon_char_features_supported(int64_t S, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo) {
    if (S < 1 || W < 1 || span < 1 || cfs < 1 || V < 1 || C < 1 || Fo < 1) return 0;
    if (span > 255 || cfs > recon::kCcMaxTaps || span + cfs - 1 > 64 || Fo > recon::kCcMaxFo || C > (1 << 16) || V > (1 << 24)) return 0;
    if (recon::cc_table_floats(cfs, V, Fo) > recon::kCcMaxTable) return 0;
    if (W > (1 << 20) || S > (static_cast<int64_t>(1) << 40) / (static_cast<int64_t>(W) * Fo)) return 0;
    return 1;
}

extern "C" size_t recon_char_features_workspace_bytes(int64_t S, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo,
                                                      int32_t backward) {
    if (S <= 0 || !recon_char_features_supported(S, W, span, cfs, V, C, Fo)) return 0;
    const int64_t n = recon::cc_table_floats(cfs, V, Fo);
    if (!backward) return align_up(static_cast<size_t>(n) * 4, 256);
    int64_t per;
    int32_t G;
    recon::cc_bwd_split(S * W, n * 4, &per, &G);
    return align_up(static_cast<size_t>(static_cast<int64_t>(G) * (n + Fo) + n) * 4, 256);
}

extern "C" int recon_char_features_fwd(const void* chars, int32_t index_bytes, int64_t ld_chars, const float* emb, const float* conv_w,
                                       const float* conv_b, const float* keep, int64_t S, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t C,
                                       int32_t Fo, float* out, uint8_t* arg_pos, void* workspace, size_t workspace_bytes, recon_stream_t stream) {
    if (S < 0 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (S == 0) return RECON_OK;
    if (!recon_char_features_supported(S, W, span, cfs, V, C, Fo)) return RECON_ERR_UNSUPPORTED;
    if (keep) return RECON_ERR_UNSUPPORTED;                             // the masked (direct) form is not built: the caller runs the op chain
    if (const int bad = recon::char_io_checks(chars && emb && conv_w && conv_b && out && workspace, ld_chars, W, span, cfs, workspace, workspace_bytes,
                                              recon_char_features_workspace_bytes(S, W, span, cfs, V, C, Fo, 0))) return bad;
    hipStream_t st = as_stream(stream);
    const int64_t n = recon::cc_table_floats(cfs, V, Fo), n_words = S * W;
    float* T = static_cast<float*>(workspace);
    hipLaunchKernelGGL(recon::k_char_tables, dim3(static_cast<unsigned>(ceil_div64(n, 256))), dim3(256), 0, st, emb, conv_w, cfs, V, C, Fo, T);
    RECON_CHECK_LAUNCH();
    const bool lds = n * 4 <= recon::kCcLdsBytes;
    const int rc = recon::dispatch_lds_ids(index_bytes, lds, [&](auto in_lds, auto id) {
        return recon::cc_launch_fwd<decltype(in_lds)::value, typename decltype(id)::type>(chars, ld_chars, T, conv_b, n_words, W, span, cfs, V, Fo, out,
                                                                                          arg_pos, st);
    });
    if (rc != RECON_OK) return rc;
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_char_features_bwd(const void* chars, int32_t index_bytes, int64_t ld_chars, const float* emb, const float* conv_w,
                                       const float* keep, const float* g_out, const float* out, const uint8_t* arg_pos, int64_t S, int32_t W,
                                       int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo, int32_t padding_idx, float* g_emb, float* g_conv_w,
                                       float* g_conv_b, void* workspace, size_t workspace_bytes, recon_stream_t stream) {
    if (S < 0 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (!recon_char_features_supported(S > 0 ? S : 1, W, span, cfs, V, C, Fo)) return RECON_ERR_UNSUPPORTED;
    if (keep) return RECON_ERR_UNSUPPORTED;
    if (!g_emb || !g_conv_w || !g_conv_b) return RECON_ERR_INVALID;
    hipStream_t st = as_stream(stream);
    if (S == 0)
        return recon::zero_fill({{g_emb, static_cast<size_t>(V) * C}, {g_conv_w, static_cast<size_t>(Fo) * C * cfs}, {g_conv_b, static_cast<size_t>(Fo)}}, st);
    if (const int bad = recon::char_io_checks(chars && emb && conv_w && g_out && out && arg_pos && workspace, ld_chars, W, span, cfs, workspace,
                                              workspace_bytes, recon_char_features_workspace_bytes(S, W, span, cfs, V, C, Fo, 1))) return bad;
    const int64_t n = recon::cc_table_floats(cfs, V, Fo), n_words = S * W;
    int64_t per;
    int32_t G;
    recon::cc_bwd_split(n_words, n * 4, &per, &G);
    float* partial = static_cast<float*>(workspace);
    float* dT = partial + static_cast<int64_t>(G) * (n + Fo);
    const bool lds = n * 4 <= recon::kCcLdsBytes;
    if (!lds && hipMemsetAsync(partial, 0, static_cast<size_t>(G) * (n + Fo) * 4, st) != hipSuccess) return RECON_ERR_LAUNCH;
    const int rc = recon::dispatch_lds_ids(index_bytes, lds, [&](auto in_lds, auto id) {
        return recon::cc_launch_bwd<decltype(in_lds)::value, typename decltype(id)::type>(chars, ld_chars, g_out, out, arg_pos, n_words, per, G, W, span, cfs,
                                                                                          V, Fo, partial, st);
    });
    if (rc != RECON_OK) return rc;
    RECON_CHECK_LAUNCH();
    hipLaunchKernelGGL(recon::k_char_reduce, dim3(static_cast<unsigned>(ceil_div64(n + Fo, 256))), dim3(256), 0, st, partial, G, static_cast<int32_t>(n), Fo,
                       dT, g_conv_b);
    RECON_CHECK_LAUNCH();
    const int64_t n_par = static_cast<int64_t>(V) * C + static_cast<int64_t>(Fo) * C * cfs;
    hipLaunchKernelGGL(recon::k_char_param_grads, dim3(static_cast<unsigned>(ceil_div64(n_par, 256))), dim3(256), 0, st, dT, emb, conv_w, cfs, V, C, Fo,
                       padding_idx, g_emb, g_conv_w);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}
