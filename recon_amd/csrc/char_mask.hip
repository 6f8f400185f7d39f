// The character CNN of csrc/char_cnn.hip (models/models.py:57-61) WITH dropout factors on the gathered embedding, the factors packed one
// bit each: factor (s, j, c) = scale if bit c % 32 of bits[s][j][c / 32] is set, else 0 (bits at and above C are ignored).
//     X[j][c]      = bit(s, j, c) ? E[chars[s][j]][c] : 0
//     pre[s][t][o] = bias[o] + scale sum_k sum_c X[t + k][c] W[o][c][k]
//     out[s][w][o] = tanh(first maximum over t in [w span, (w + 1) span) of pre[s][t][o])
// The mask breaks the table form (the sum over c no longer depends on the id alone): this is a real fp32 convolution.  Nothing of size
// S Lc C is written; the masked rows of ONE word live in LDS while the word is worked on.
//
// k_keep_bits_draw: the bits from Philox4x32-10, one thread per character position (the definition is in include/recon_hip.h).
// k_char_masked_prep: the filter bank as the B operand Wr[kk][o], kk = k C + c, rows padded with zeros to a multiple of 4 and the row
//   pitch chosen = 16 (mod 32) floats, so that the four k rows of a B fragment fall into different banks.
// k_char_masked_fwd: ONE WAVE PER WORD on v_mfma_f32_16x16x4_f32 (exact fp32: a k-ordered fma chain).  The wave writes the word's masked
//   rows Xs[j][c] with row pitch exactly C; then im2col costs nothing, row p of the A operand is the cfs C consecutive floats behind
//   Xs[p][0].  A tile is 16 window positions x 16 output channels; 4 channel tiles share one A fragment.  The lanes' accumulators hold 4
//   positions of one channel each: the first maximum is taken per lane in position order, then across the four lane groups (the lower
//   position wins a tie).  E and Wr lie in LDS while they fit (144 KiB with the row tiles), else they are read through L2 by the same code.
// k_char_masked_bwd: d_pre = g_out (1 - out^2) at the saved position only.  No floating-point atomics.  Workgroup g owns a fixed run of
//   words and private dE [V][C], dW [Fo][cfs][C], db [Fo] (LDS while they fit, else its slab of the workspace, zeroed by the host call).
//   Lane = c; wave w owns the output channels o = w (mod 4): it alone writes dW[o] and its own partial dX tile; after a barrier the four
//   partial tiles are added in wave order; then wave w adds the rows whose ID is = w (mod 4) to dE, in row order (ownership by id: two
//   rows of a word can hold the same id).  The next word's ids, bits, g_out, out and positions are loaded before the current word's
//   arithmetic.  k_char_masked_reduce adds the slabs in workgroup order and writes g_conv_w in its [Fo][C][cfs] layout.
#include <math.h>
#include "ctx_enc_common.h"

namespace recon {
namespace {

constexpr int kCmMaxFo = 256;
constexpr int kCmMaxTaps = 16;
constexpr int kCmMaxC = 64;                    // one lane per embedding channel, two bit words
constexpr int kCmLdsBytes = 144 * 1024;
constexpr int64_t kCmMaxSlab = 1 << 22;        // floats of one private accumulator set
constexpr int kCmBwdMinWords = 16;
constexpr int kCmBwdMaxWg = 256;

struct CmFwdGeo { int32_t Kp, FoP, pitch, n_pt, xs_floats; };
inline CmFwdGeo cm_fwd_geo(int32_t span, int32_t cfs, int32_t C, int32_t Fo) {
    CmFwdGeo g;
    g.Kp = (cfs * C + 3) / 4 * 4;
    g.FoP = (Fo + 15) / 16 * 16;
    g.pitch = g.FoP % 32 == 16 ? g.FoP : g.FoP + 16;
    g.n_pt = (span + 15) / 16;
    g.xs_floats = ((g.n_pt * 16 + cfs) * C + 4 + 3) / 4 * 4;         // the A fragment of the last tile reads up to Kp - 1 behind its row
    return g;
}
inline int64_t cm_slab_floats(int32_t cfs, int32_t V, int32_t C, int32_t Fo) {
    return static_cast<int64_t>(V) * C + static_cast<int64_t>(Fo) * cfs * C + Fo;
}
// floats of LDS the backward needs beside the accumulators: Xs, the summed dX, four partial dX tiles, d_pre and positions of a word
inline int64_t cm_bwd_small_floats(int32_t span, int32_t cfs, int32_t C, int32_t Fo) {
    return 6 * static_cast<int64_t>(span + cfs - 1) * C + 2 * Fo;
}

// ---- Philox4x32-10 ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c[0], p1 = static_cast<uint64_t>(0xCD9E8D57u) * c[2];
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c[1] ^ k0, n2 = static_cast<uint32_t>(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = static_cast<uint32_t>(p1); c[2] = n2; c[3] = static_cast<uint32_t>(p0);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

__global__ void __launch_bounds__(256) k_keep_bits_draw(uint32_t* __restrict__ bits, int64_t n_positions, int32_t C, uint32_t threshold,
                                                        uint64_t seed, uint64_t offset) {
    const int64_t q = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (q >= n_positions) return;
    const int KW = (C + 31) >> 5, Gp = (C + 3) >> 2;
    const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
    for (int kw = 0; kw < KW; ++kw) {
        uint32_t word = 0;
        for (int g8 = 0; g8 < 8 && kw * 8 + g8 < Gp; ++g8) {
            const int g = kw * 8 + g8;
            const uint64_t ctr = offset + static_cast<uint64_t>(q) * Gp + g;
            uint32_t r[4] = {static_cast<uint32_t>(ctr), static_cast<uint32_t>(ctr >> 32), 0u, 0u};
            philox4x32_10(r, k0, k1);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * g + i < C && r[i] >= threshold) word |= 1u << (4 * g8 + i);
        }
        bits[q * KW + kw] = word;
    }
}

__global__ void __launch_bounds__(256) k_char_masked_prep(const float* __restrict__ Wc, int32_t cfs, int32_t C, int32_t Fo, int32_t Kp,
                                                          int32_t pitch, float* __restrict__ Wr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Kp * pitch) return;
    const int o = i % pitch, kk = i / pitch;
    float v = 0.f;
    if (o < Fo && kk < cfs * C) {
        const int k = kk / C, c = kk - k * C;
        v = Wc[(static_cast<int64_t>(o) * C + c) * cfs + k];
    }
    Wr[i] = v;
}

template <bool LDS, typename IdT>
__global__ void __launch_bounds__(512) k_char_masked_fwd(const IdT* __restrict__ chars, int64_t ld_chars, const float* __restrict__ E,
                                                         const float* __restrict__ Wr, const float* __restrict__ bias,
                                                         const uint32_t* __restrict__ bits, float scale, int64_t n_words, int32_t W,
                                                         int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo, int32_t Kp,
                                                         int32_t pitch, int32_t xs_floats, float* __restrict__ out,
                                                         uint8_t* __restrict__ arg) {
    extern __shared__ float cm_lds[];
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6, nw = blockDim.x >> 6;
    float* xs = cm_lds + wid * xs_floats;
    const float* wr = Wr;
    const float* emb = E;
    for (int i = t; i < nw * xs_floats; i += blockDim.x) cm_lds[i] = 0.f;       // the tails behind the rows stay zero for good
    if constexpr (LDS) {
        float* lw = cm_lds + nw * xs_floats;
        float* le = lw + Kp * pitch;
        for (int i = t; i < Kp * pitch; i += blockDim.x) lw[i] = Wr[i];
        for (int i = t; i < V * C; i += blockDim.x) le[i] = E[i];
        wr = lw;
        emb = le;
    }
    __syncthreads();
    const int n_ids = span + cfs - 1, KW = (C + 31) >> 5, n_pt = (span + 15) >> 4, FoP = (Fo + 15) & ~15;
    const int64_t Lc = cfs - 1 + static_cast<int64_t>(W) * span;
    const int64_t n_waves = static_cast<int64_t>(gridDim.x) * nw;
    const int grp = lane >> 4, col = lane & 15;
    int idv_n = 0;
    uint32_t bw0_n = 0, bw1_n = 0;
    auto fetch = [&](int64_t word) {                                            // ids and bit words of a word: row j in lane j
        const int64_t s = word / W;
        const int w = static_cast<int>(word - s * W);
        idv_n = word_ids(chars + s * ld_chars + static_cast<int64_t>(w) * span, lane, n_ids, V);
        const int64_t pos = s * Lc + static_cast<int64_t>(w) * span + (lane < n_ids ? lane : 0);
        bw0_n = bits[pos * KW];
        bw1_n = bits[pos * KW + KW - 1];
    };
    const int64_t first = static_cast<int64_t>(blockIdx.x) * nw + wid;
    if (first < n_words) fetch(first);
    for (int64_t word = first; word < n_words; word += n_waves) {
        const int idv = idv_n;
        const uint32_t bw0 = bw0_n, bw1 = bw1_n;
        if (word + n_waves < n_words) fetch(word + n_waves);                    // the next word's loads fly during this word's arithmetic
        // (the wave's own reads of the previous word precede these writes in program order: LDS serves a wave in order)
        for (int j0 = 0; j0 < n_ids; j0 += 4) {                                 // four rows' reads before their writes
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = min(j0 + u, n_ids - 1);
                const int id = __builtin_amdgcn_readlane(idv, j);
                const uint32_t b0 = __builtin_amdgcn_readlane(bw0, j), b1 = __builtin_amdgcn_readlane(bw1, j);
                const uint32_t bw = lane < 32 ? b0 : b1;
                v[u] = (lane < C && ((bw >> (lane & 31)) & 1u)) ? emb[id * C + lane] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (j0 + u < n_ids && lane < C) xs[(j0 + u) * C + lane] = v[u];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int ob = 0; ob < Fo; ob += 64) {
            float best[4], bsv[4];
            int bp[4], co[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                best[q] = -INFINITY;
                bp[q] = 255;
                co[q] = min(ob + 16 * q, FoP - 16);                             // a tile past Fo repeats the last one and is not stored
                bsv[q] = bias[min(co[q] + col, Fo - 1)];
            }
            for (int pt = 0; pt < n_pt; ++pt) {
                enc_f32x4 acc[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = enc_f32x4{0.f, 0.f, 0.f, 0.f};
                const float* ap = xs + (pt * 16 + col) * C + grp;
                const float* bq = wr + grp * pitch + col;
                int kk = 0;
                for (; kk + 8 <= Kp; kk += 8) {                                 // two k steps' operands are read before the first product
                    const float a0 = ap[kk], a1 = ap[kk + 4];
                    const float* br = bq + kk * pitch;
                    float b0[4], b1[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { b0[q] = br[co[q]]; b1[q] = br[4 * pitch + co[q]]; }
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0[q], acc[q], 0, 0, 0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1[q], acc[q], 0, 0, 0);
                }
                if (kk < Kp) {
                    const float a = ap[kk];
                    const float* br = bq + kk * pitch;
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, br[co[q]], acc[q], 0, 0, 0);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int p = pt * 16 + grp * 4 + i;
                        const float v = fmaf(scale, acc[q][i], bsv[q]);
                        if (p < span && (p == 0 || v > best[q])) { best[q] = v; bp[q] = p; }
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int off = 16; off <= 32; off <<= 1) {
                    const float ov = __shfl_xor(best[q], off, 64);
                    const int op = __shfl_xor(bp[q], off, 64);
                    if (ov > best[q] || (ov == best[q] && op < bp[q])) { best[q] = ov; bp[q] = op; }     // a tie goes to the lower position
                }
                const int o = ob + 16 * q + col;
                if (grp == 0 && o < Fo) {
                    const int64_t at = word * Fo + o;
                    out[at] = tanhf(best[q]);
                    if (arg) arg[at] = static_cast<uint8_t>(bp[q]);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

template <bool LDS, typename IdT>
__global__ void __launch_bounds__(256) k_char_masked_bwd(const IdT* __restrict__ chars, int64_t ld_chars, const float* __restrict__ E,
                                                         const float* __restrict__ Wc, const uint32_t* __restrict__ bits, float scale,
                                                         const float* __restrict__ g_out, const float* __restrict__ out,
                                                         const uint8_t* __restrict__ arg, int64_t n_words, int64_t words_per_wg, int32_t W,
                                                         int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo, int32_t padding_idx,
                                                         float* __restrict__ partial) {
    extern __shared__ float cm_lds[];
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int n_ids = span + cfs - 1, KW = (C + 31) >> 5, tile = n_ids * C, nE = V * C, nW = Fo * cfs * C;
    const int64_t Lc = cfs - 1 + static_cast<int64_t>(W) * span;
    float* slab = partial + static_cast<int64_t>(blockIdx.x) * (nE + nW + Fo);  // dE [V][C], dW [Fo][cfs][C], db [Fo]
    float* xs = cm_lds;
    float* dxs = xs + tile;
    float* dxw = dxs + tile;
    float* dsh = dxw + 4 * tile;
    int* tsh = reinterpret_cast<int*>(dsh + Fo);
    float* dE = slab;
    float* dWl = slab + nE;
    const float* wl = nullptr;
    const float* emb = E;
    if constexpr (LDS) {
        dE = dsh + 2 * Fo;
        dWl = dE + nE;
        float* w_ = dWl + nW;
        float* e_ = w_ + nW;
        for (int i = t; i < nE + nW; i += 256) dE[i] = 0.f;
        for (int i = t; i < nW; i += 256) {
            const int c = i % C, k = (i / C) % cfs, o = i / (C * cfs);
            w_[i] = Wc[(static_cast<int64_t>(o) * C + c) * cfs + k];
        }
        for (int i = t; i < nE; i += 256) e_[i] = E[i];
        wl = w_;
        emb = e_;
    }
    __syncthreads();
    const int64_t w0 = static_cast<int64_t>(blockIdx.x) * words_per_wg, w1 = min64(w0 + words_per_wg, n_words);
    float db = 0.f;
    int idv_n = 0;
    uint32_t bw0_n = 0, bw1_n = 0;
    float g_n = 0.f, y_n = 0.f;
    int a_n = 0;
    auto fetch = [&](int64_t word) {
        const int64_t s = word / W;
        const int w = static_cast<int>(word - s * W);
        idv_n = word_ids(chars + s * ld_chars + static_cast<int64_t>(w) * span, lane, n_ids, V);
        const int64_t pos = s * Lc + static_cast<int64_t>(w) * span + (lane < n_ids ? lane : 0);
        bw0_n = bits[pos * KW];
        bw1_n = bits[pos * KW + KW - 1];
        if (t < Fo) {
            const int64_t at = word * Fo + t;
            g_n = g_out[at];
            y_n = out[at];
            a_n = arg[at];
        }
    };
    if (w0 < w1) fetch(w0);
    for (int64_t word = w0; word < w1; ++word) {
        const int idv = idv_n;
        const uint32_t bw0 = bw0_n, bw1 = bw1_n;
        const float g = g_n, y = y_n;
        const int a = a_n;
        if (word + 1 < w1) fetch(word + 1);
        if (t < Fo) {
            const float d = g * (1.f - y * y);
            db += d;
            dsh[t] = d * scale;
            tsh[t] = min(a, span - 1);
        }
        for (int j = wid; j < n_ids; j += 4) {
            const int id = __builtin_amdgcn_readlane(idv, j);
            const uint32_t b0 = __builtin_amdgcn_readlane(bw0, j), b1 = __builtin_amdgcn_readlane(bw1, j);
            const uint32_t bw = lane < 32 ? b0 : b1;
            if (lane < C) xs[j * C + lane] = ((bw >> (lane & 31)) & 1u) ? emb[id * C + lane] : 0.f;
        }
        float* mine = dxw + wid * tile;
        for (int i = lane; i < tile; i += 64) mine[i] = 0.f;
        __syncthreads();
        if (lane < C) {
            for (int o = wid; o < Fo; o += 4) {
                const float d = dsh[o];
                const int ts = tsh[o];
                for (int k = 0; k < cfs; ++k) {
                    const int r = (ts + k) * C + lane, cell = (o * cfs + k) * C + lane;
                    dWl[cell] = fmaf(d, xs[r], dWl[cell]);
                    const float wv = LDS ? wl[cell] : Wc[(static_cast<int64_t>(o) * C + lane) * cfs + k];
                    mine[r] = fmaf(d, wv, mine[r]);
                }
            }
        }
        __syncthreads();
        for (int i = t; i < tile; i += 256) dxs[i] = ((dxw[i] + dxw[tile + i]) + dxw[2 * tile + i]) + dxw[3 * tile + i];
        __syncthreads();
        for (int j = 0; j < n_ids; ++j) {
            const int id = __builtin_amdgcn_readlane(idv, j);
            if ((id & 3) != wid || id == padding_idx) continue;
            const uint32_t b0 = __builtin_amdgcn_readlane(bw0, j), b1 = __builtin_amdgcn_readlane(bw1, j);
            const uint32_t bw = lane < 32 ? b0 : b1;
            if (lane < C && ((bw >> (lane & 31)) & 1u)) dE[id * C + lane] += dxs[j * C + lane];
        }
    }
    if (t < Fo) slab[nE + nW + t] = db;
    if constexpr (LDS) {
        __syncthreads();
        for (int i = t; i < nE + nW; i += 256) slab[i] = dE[i];
    }
}

// the G slabs added in slab order: g_emb [V][C], g_conv_w [Fo][C][cfs] from the slab's [Fo][cfs][C], g_conv_b [Fo]
__global__ void __launch_bounds__(256) k_char_masked_reduce(const float* __restrict__ partial, int32_t G, int32_t cfs, int32_t V, int32_t C,
                                                            int32_t Fo, float* __restrict__ g_emb, float* __restrict__ g_w,
                                                            float* __restrict__ g_b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int nE = V * C, nW = Fo * cfs * C, n = nE + nW + Fo;
    if (i >= n) return;
    float sum = 0.f;
#pragma unroll 8
    for (int g = 0; g < G; ++g) sum += partial[static_cast<int64_t>(g) * n + i];
    if (i < nE) {
        g_emb[i] = sum;
    } else if (i < nE + nW) {
        const int r = i - nE, c = r % C, k = (r / C) % cfs, o = r / (C * cfs);
        g_w[(static_cast<int64_t>(o) * C + c) * cfs + k] = sum;
    } else {
        g_b[i - nE - nW] = sum;
    }
}

template <bool LDS, typename IdT>
int cm_launch_fwd(const void* chars, int64_t ld_chars, const float* E, const float* Wr, const float* bias, const uint32_t* bits, float scale,
                  int64_t n_words, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo, const CmFwdGeo& g, int nw,
                  float* out, uint8_t* arg, hipStream_t st) {
    const size_t lds = (static_cast<size_t>(nw) * g.xs_floats + (LDS ? static_cast<size_t>(g.Kp) * g.pitch + static_cast<size_t>(V) * C : 0)) * 4;
    auto kern = &k_char_masked_fwd<LDS, IdT>;
    if (!allow_lds(kern, lds)) return RECON_ERR_LAUNCH;
    const int64_t blocks = LDS ? min64(ceil_div64(n_words, 4 * nw), 256) : min64(ceil_div64(n_words, nw), 2048);
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks)), dim3(64 * nw), lds, st, static_cast<const IdT*>(chars), ld_chars, E, Wr, bias, bits,
                       scale, n_words, W, span, cfs, V, C, Fo, g.Kp, g.pitch, g.xs_floats, out, arg);
    return RECON_OK;
}

template <bool LDS, typename IdT>
int cm_launch_bwd(const void* chars, int64_t ld_chars, const float* E, const float* Wc, const uint32_t* bits, float scale, const float* g_out,
                  const float* out, const uint8_t* arg, int64_t n_words, int64_t per, int32_t G, int32_t W, int32_t span, int32_t cfs, int32_t V,
                  int32_t C, int32_t Fo, int32_t padding_idx, float* partial, hipStream_t st) {
    const int64_t nE = static_cast<int64_t>(V) * C, nW = static_cast<int64_t>(Fo) * cfs * C;
    const size_t lds = static_cast<size_t>(cm_bwd_small_floats(span, cfs, C, Fo) + (LDS ? 2 * (nE + nW) : 0)) * 4;
    auto kern = &k_char_masked_bwd<LDS, IdT>;
    if (!allow_lds(kern, lds)) return RECON_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(G)), dim3(256), lds, st, static_cast<const IdT*>(chars), ld_chars, E, Wc, bits, scale, g_out,
                       out, arg, n_words, per, W, span, cfs, V, C, Fo, padding_idx, partial);
    return RECON_OK;
}

}  // namespace
}  // namespace recon

extern "C" int recon_char_masked_supported(int64_t S, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo) {
    if (S < 1 || W < 1 || span < 1 || cfs < 1 || V < 1 || C < 1 || Fo < 1) return 0;
    if (span > 255 || cfs > recon::kCmMaxTaps || span + cfs - 1 > 64 || Fo > recon::kCmMaxFo || C > recon::kCmMaxC || V > (1 << 24)) return 0;
    if (recon::cm_slab_floats(cfs, V, C, Fo) > recon::kCmMaxSlab) return 0;
    if (W > (1 << 20) || S > (static_cast<int64_t>(1) << 40) / (static_cast<int64_t>(W) * Fo)) return 0;
    return 1;
}

extern "C" size_t recon_char_masked_workspace_bytes(int64_t S, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo,
                                                    int32_t backward) {
    if (S <= 0 || !recon_char_masked_supported(S, W, span, cfs, V, C, Fo)) return 0;
    if (!backward) {
        const recon::CmFwdGeo g = recon::cm_fwd_geo(span, cfs, C, Fo);
        return align_up(static_cast<size_t>(g.Kp) * g.pitch * 4, 256);
    }
    int64_t per;
    int32_t G;
    recon::split_rows(S * W, recon::kCmBwdMaxWg, recon::kCmBwdMinWords, &per, &G);
    return align_up(static_cast<size_t>(G) * recon::cm_slab_floats(cfs, V, C, Fo) * 4, 256);
}

extern "C" int recon_char_keep_bits_draw(int32_t* bits, int64_t n_positions, int32_t C, uint32_t threshold_u32, uint64_t seed_u64,
                                         uint64_t offset_u64, recon_stream_t stream) {
    if (n_positions < 0 || C < 1 || C > (1 << 16)) return RECON_ERR_INVALID;
    if (n_positions == 0) return RECON_OK;
    if (!bits || n_positions > (static_cast<int64_t>(1) << 38)) return RECON_ERR_INVALID;
    hipLaunchKernelGGL(recon::k_keep_bits_draw, dim3(static_cast<unsigned>(ceil_div64(n_positions, 256))), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<uint32_t*>(bits), n_positions, C, threshold_u32, seed_u64, offset_u64);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_char_masked_fwd(const void* chars, int32_t index_bytes, int64_t ld_chars, const float* emb, const float* conv_w,
                                     const float* conv_b, const int32_t* bits, float scale, int64_t S, int32_t W, int32_t span, int32_t cfs,
                                     int32_t V, int32_t C, int32_t Fo, float* out, uint8_t* arg_pos, void* workspace, size_t workspace_bytes,
                                     recon_stream_t stream) {
    if (S < 0 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (S == 0) return RECON_OK;
    if (!recon_char_masked_supported(S, W, span, cfs, V, C, Fo)) return RECON_ERR_UNSUPPORTED;
    if (const int bad = recon::char_io_checks(chars && emb && conv_w && conv_b && bits && out && workspace, ld_chars, W, span, cfs, workspace,
                                              workspace_bytes, recon_char_masked_workspace_bytes(S, W, span, cfs, V, C, Fo, 0))) return bad;
    hipStream_t st = as_stream(stream);
    const recon::CmFwdGeo g = recon::cm_fwd_geo(span, cfs, C, Fo);
    float* Wr = static_cast<float*>(workspace);
    hipLaunchKernelGGL(recon::k_char_masked_prep, dim3(static_cast<unsigned>(ceil_div64(static_cast<int64_t>(g.Kp) * g.pitch, 256))), dim3(256), 0, st,
                       conv_w, cfs, C, Fo, g.Kp, g.pitch, Wr);
    RECON_CHECK_LAUNCH();
    const int64_t tables = static_cast<int64_t>(g.Kp) * g.pitch + static_cast<int64_t>(V) * C;
    const bool lds = (tables + 4 * g.xs_floats) * 4 <= recon::kCmLdsBytes;
    const int nw = ((lds ? tables : 0) + 8 * g.xs_floats) * 4 <= recon::kCmLdsBytes ? 8 : 4;
    const uint32_t* b = reinterpret_cast<const uint32_t*>(bits);
    const int64_t n_words = S * W;
    const int rc = recon::dispatch_lds_ids(index_bytes, lds, [&](auto in_lds, auto id) {
        return recon::cm_launch_fwd<decltype(in_lds)::value, typename decltype(id)::type>(chars, ld_chars, emb, Wr, conv_b, b, scale, n_words, W, span, cfs, V,
                                                                                          C, Fo, g, nw, out, arg_pos, st);
    });
    if (rc != RECON_OK) return rc;
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_char_masked_bwd(const void* chars, int32_t index_bytes, int64_t ld_chars, const float* emb, const float* conv_w,
                                     const int32_t* bits, float scale, const float* g_out, const float* out, const uint8_t* arg_pos, int64_t S,
                                     int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo, int32_t padding_idx, float* g_emb,
                                     float* g_conv_w, float* g_conv_b, void* workspace, size_t workspace_bytes, recon_stream_t stream) {
    if (S < 0 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (!recon_char_masked_supported(S > 0 ? S : 1, W, span, cfs, V, C, Fo)) return RECON_ERR_UNSUPPORTED;
    if (!g_emb || !g_conv_w || !g_conv_b) return RECON_ERR_INVALID;
    hipStream_t st = as_stream(stream);
    if (S == 0)
        return recon::zero_fill({{g_emb, static_cast<size_t>(V) * C}, {g_conv_w, static_cast<size_t>(Fo) * C * cfs}, {g_conv_b, static_cast<size_t>(Fo)}}, st);
    if (const int bad = recon::char_io_checks(chars && emb && conv_w && bits && g_out && out && arg_pos && workspace, ld_chars, W, span, cfs, workspace,
                                              workspace_bytes, recon_char_masked_workspace_bytes(S, W, span, cfs, V, C, Fo, 1))) return bad;
    const int64_t n_words = S * W, slab = recon::cm_slab_floats(cfs, V, C, Fo);
    int64_t per;
    int32_t G;
    recon::split_rows(n_words, recon::kCmBwdMaxWg, recon::kCmBwdMinWords, &per, &G);
    float* partial = static_cast<float*>(workspace);
    const bool lds = (recon::cm_bwd_small_floats(span, cfs, C, Fo) + 2 * (slab - Fo)) * 4 <= recon::kCmLdsBytes;
    if (!lds && hipMemsetAsync(partial, 0, static_cast<size_t>(G) * slab * 4, st) != hipSuccess) return RECON_ERR_LAUNCH;
    const uint32_t* b = reinterpret_cast<const uint32_t*>(bits);
    const int rc = recon::dispatch_lds_ids(index_bytes, lds, [&](auto in_lds, auto id) {
        return recon::cm_launch_bwd<decltype(in_lds)::value, typename decltype(id)::type>(chars, ld_chars, emb, conv_w, b, scale, g_out, out, arg_pos, n_words, per,
                                                                                          G, W, span, cfs, V, C, Fo, padding_idx, partial, st);
    });
    if (rc != RECON_OK) return rc;
    RECON_CHECK_LAUNCH();
    hipLaunchKernelGGL(recon::k_char_masked_reduce, dim3(static_cast<unsigned>(ceil_div64(slab, 256))), dim3(256), 0, st, partial, G, cfs, V, C, Fo, g_emb,
                       g_conv_w, g_conv_b);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}
