// The entity-context line LSTM (models/models.py:56-70): one layer, two directions, batch_first, S independent sequences of exactly T
// steps, only the two final hidden states kept:   out[s] = (h_fwd after t = T - 1 | h_rev after t = 0).
//     x[s][t]   = (word_table[words[s][t]] | feat[s][t][:Fc])                       (I = Dw + Fc; the concatenation is never written)
//     a[s][t]   = W_ih x[s][t] + b_ih + W_hh h[s][t'] + b_hh,  t' the step before t in the direction's walk, h = c = 0 in front of it
//     i, f, o   = sigmoid(a[0:H], a[H:2H], a[3H:4H]),  g = tanh(a[2H:3H]),  c[t] = f c[t'] + i g,  h[t] = o tanh(c[t])
// Everything is fp32 on v_mfma_f32_16x16x4_f32 (an fp32 fma chain in k order); no floating-point atomics, every sum has one order.
//
// k_ctx_lstm_prep: both directions' weights as the forward's B operand Wr[kk][q H + u] (kk < Kx: W_ih^T, zero rows up to Kx = 4 ceil(I/4);
//   then W_hh^T, zero rows up to Kh), row pitch = 16 (mod 32) floats so that the two k rows a half-wave reads fall into different banks,
//   followed by b_ih + b_hh.
// k_ctx_lstm_fwd: a workgroup owns one direction and walks tiles of 16 sequences.  Wr lies in LDS for good.  Wave b computes the four gate
//   tiles of the hidden units [16 b, 16 b + 16): i, f, g, o of one (sequence, unit) land in the same lane of the four accumulators, c never
//   leaves registers, h[t] goes back through LDS (two buffers) for the next step.  The next step's ids and input rows are fetched into
//   registers under the current step's products.  With `saved` it writes (i, f, g, o, c) of every step: 5 H floats per (direction, s, t).
// k_ctx_lstm_bptt: one launch per direction (d_x is the sum over both: the second launch adds to what the first wrote); per tile the steps
//   backwards, W = (W_ih | W_hh) in its own layout [4H][I + H] as the B operand.  d_h and
//   d_c stay in registers in the forward's lane layout; the step's d_a goes through LDS as the A operand; wave b's first output tile is
//   d_h of its own units, the others are columns of d_x, written to d_word_vec / d_feat.  It leaves d_a where the gates were and h[t]
//   where c[t] was.
// k_ctx_lstm_wgrad: workgroup g owns a fixed run of sequences and accumulates d_a^T . (x | h[t'] | 1) over its (s, t) rows, 16 at a time
//   through LDS, every output tile in the registers of one wave; the column of ones gives the bias gradient.  k_lstm_reduce (lstm_common.h,
//   with Vp = 0 and no class sums) adds the slabs in workgroup order and scatters into the eight gradients.
#include "lstm_common.h"

namespace recon {
namespace {

constexpr int kClLdsFloats = 144 * 1024 / 4;
constexpr int kClMaxH = 64;                    // four waves, one 16-unit block each
constexpr int kClMaxI = 256;                   // 16 staged floats per thread and row
constexpr int kClMaxWg = 128;                  // workgroups per direction (the BPTT pass, one direction per launch: twice as many)
constexpr int kClSlots = 48;                   // dW tiles one wave of the weight-gradient pass holds

struct ClGeo {
    int32_t I, Kx, Kh, pB, pX, pH;             // forward
    int32_t K4, pW, pG;                        // BPTT
    int32_t MT, NT, N, pGs, pXs;               // weight gradient
    int64_t fwd_floats, bptt_floats, wg_floats;
};
inline ClGeo cl_geo(int32_t Dw, int32_t Fc, int32_t H) {
    ClGeo g;
    g.I = Dw + Fc;
    g.Kx = (g.I + 3) / 4 * 4;
    g.Kh = (H + 3) / 4 * 4;
    g.pB = lstm_pitch(4 * H, 16);
    g.pX = lstm_pitch(g.Kx, 2);                   // A rows: 16 sequences x 2 k of a half-wave in 32 different banks
    g.pH = lstm_pitch(g.Kh, 2);
    g.fwd_floats = static_cast<int64_t>(g.Kx + g.Kh) * g.pB + 16 * g.pX + 32 * g.pH;
    g.K4 = 4 * H;                               // (a multiple of 4 already)
    g.pG = lstm_pitch(g.K4, 2);
    g.pW = lstm_pitch(g.I + H, 16);
    if (static_cast<int64_t>(g.K4) * g.pW + 16 * g.pG > kClLdsFloats) g.pW = (g.I + H) % 32 ? g.I + H : g.I + H + 1;      // compact: some 2-way conflicts
    g.bptt_floats = static_cast<int64_t>(g.K4) * g.pW + 16 * g.pG;
    g.N = g.I + H + 1;
    g.MT = (4 * H + 15) / 16;
    g.NT = (g.N + 15) / 16;
    g.pGs = lstm_pitch(16 * g.MT, 16);
    g.pXs = lstm_pitch(16 * g.NT, 16);
    g.wg_floats = 2 * 16 * static_cast<int64_t>(g.pGs + g.pXs);
    return g;
}

// acc[q] += A[16 x K] . B[K x 16 at column cq[q]], K a multiple of 4; two k steps' operands are read before the first product
__device__ __forceinline__ void cl_gate_products(const float* ap, const float* bq, int pitch, const int (&cq)[4], int K, enc_f32x4 (&acc)[4]) {
    int kk = 0;
    for (; kk + 8 <= K; kk += 8) {
        const float a0 = ap[kk], a1 = ap[kk + 4];
        const float* br = bq + kk * pitch;
        float b0[4], b1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { b0[q] = br[cq[q]]; b1[q] = br[4 * pitch + cq[q]]; }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0[q], acc[q], 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1[q], acc[q], 0, 0, 0);
    }
    if (kk < K) {
        const float a = ap[kk];
        const float* br = bq + kk * pitch;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, br[cq[q]], acc[q], 0, 0, 0);
    }
}

__global__ void __launch_bounds__(256) k_ctx_lstm_prep(const float* __restrict__ w_ih_f, const float* __restrict__ w_hh_f,
                                                       const float* __restrict__ b_ih_f, const float* __restrict__ b_hh_f,
                                                       const float* __restrict__ w_ih_r, const float* __restrict__ w_hh_r,
                                                       const float* __restrict__ b_ih_r, const float* __restrict__ b_hh_r, int32_t I, int32_t H,
                                                       int32_t Kx, int32_t Kh, int32_t pB, float* __restrict__ Wr) {
    const int per = (Kx + Kh) * pB + 4 * H;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * per) return;
    const int dir = i / per, r = i - dir * per;
    const float* w_ih = dir ? w_ih_r : w_ih_f;
    const float* w_hh = dir ? w_hh_r : w_hh_f;
    float v = 0.f;
    if (r >= (Kx + Kh) * pB) {
        const int j = r - (Kx + Kh) * pB;
        v = (dir ? b_ih_r : b_ih_f)[j] + (dir ? b_hh_r : b_hh_f)[j];
    } else {
        const int kk = r / pB, j = r - kk * pB;
        if (j < 4 * H) {
            if (kk < I) v = w_ih[static_cast<int64_t>(j) * I + kk];
            else if (kk >= Kx && kk - Kx < H) v = w_hh[static_cast<int64_t>(j) * H + (kk - Kx)];
        }
    }
    Wr[i] = v;
}

template <typename IdT>
__global__ void __launch_bounds__(256) k_ctx_lstm_fwd(const IdT* __restrict__ words, int64_t ld_words, const float* __restrict__ table, int32_t Vw,
                                                      const float* __restrict__ feat, int64_t ld_feat, const float* __restrict__ Wr, int64_t S,
                                                      int32_t T, int32_t Dw, int32_t Fc, int32_t H, int32_t Kx, int32_t Kh, int32_t pB, int32_t pX,
                                                      int32_t pH, float* __restrict__ out, float* __restrict__ saved) {
    extern __shared__ float cl_lds[];
    const int t = threadIdx.x, lane = t & 63, wid = __builtin_amdgcn_readfirstlane(t >> 6), grp = lane >> 4, col = lane & 15;
    const int dir = blockIdx.y, I = Dw + Fc, rows = Kx + Kh;
    float* wl = cl_lds;
    float* xs = wl + rows * pB;
    float* hs = xs + 16 * pX;                                                   // [2][16][pH]
    const float* wsrc = Wr + static_cast<int64_t>(dir) * (rows * pB + 4 * H);
    for (int i = t; i < rows * pB; i += 256) wl[i] = wsrc[i];
    for (int i = t; i < 16 * pX + 32 * pH; i += 256) xs[i] = 0.f;               // the tails behind I and H stay zero for good
    const int u = 16 * wid + col, uc = min(u, H - 1);
    const bool active = 16 * wid < H;
    float bias[4];
    int cq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        cq[q] = q * H + uc;
        bias[q] = wsrc[rows * pB + cq[q]];
    }
    __syncthreads();
    const int lr = t >> 4, lc = t & 15;
    const int64_t n_tiles = (S + 15) / 16;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t s0 = tile * 16, srow = s0 + lr;
        const bool sv = srow < S;
        float xv[16];
        auto load_x = [&](int tt) {                                             // row lr of step tt: columns lc, lc + 16, ...
            int id = 0;
            if (Dw > 0 && sv) id = lstm_id(words + srow * ld_words + tt, Vw);
            const float* trow = table + static_cast<int64_t>(id) * Dw;
            const float* frow = feat + (srow * T + tt) * ld_feat - Dw;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int c = lc + 16 * j;
                float v = 0.f;
                if (sv && c < I) v = c < Dw ? trow[c] : frow[c];
                xv[j] = v;
            }
        };
        auto store_x = [&]() {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int c = lc + 16 * j;
                if (c < I) xs[lr * pX + c] = xv[j];
            }
        };
        load_x(dir ? T - 1 : 0);
        store_x();
        for (int i = t; i < 16 * pH; i += 256) hs[i] = 0.f;                     // h in front of the first step
        float c[4] = {0.f, 0.f, 0.f, 0.f};
        __syncthreads();
        for (int k = 0; k < T; ++k) {
            const int tt = dir ? T - 1 - k : k;
            if (k + 1 < T) load_x(dir ? tt - 1 : tt + 1);                       // flies during this step's products
            const float* hc = hs + (k & 1) * 16 * pH;
            float* hn = hs + ((k & 1) ^ 1) * 16 * pH;
            if (active) {
                enc_f32x4 acc[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = enc_f32x4{0.f, 0.f, 0.f, 0.f};
                const float* ap = xs + col * pX + grp;
                const float* bq = wl + grp * pB;
                cl_gate_products(ap, bq, pB, cq, Kx, acc);
                ap = hc + col * pH + grp;
                bq = wl + (Kx + grp) * pB;
                cl_gate_products(ap, bq, pB, cq, Kh, acc);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = 4 * grp + i;
                    float ig, fg, gg, og;
                    const float h = lstm_cell_fwd(acc[0][i], acc[1][i], acc[2][i], acc[3][i], bias, c[i], ig, fg, gg, og);
                    if (u < H) {
                        hn[m * pH + u] = h;
                        if (s0 + m < S) {
                            if (saved) {
                                float* sp = lstm_saved_row(saved, static_cast<int64_t>(dir) * S + s0 + m, T, tt, lstm_row_floats(H)) + u;
                                lstm_cell_store(sp, H, ig, fg, gg, og, c[i]);
                            }
                            if (k == T - 1) out[(s0 + m) * (2 * H) + dir * H + u] = h;
                        }
                    }
                }
            }
            __syncthreads();                                                    // every wave is done with xs and hc; hn is complete
            if (k + 1 < T) store_x();
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(256) k_ctx_lstm_bptt(const float* __restrict__ w_ih_f, const float* __restrict__ w_hh_f,
                                                       const float* __restrict__ w_ih_r, const float* __restrict__ w_hh_r,
                                                       const float* __restrict__ g_out, float* __restrict__ saved, int64_t S, int32_t T, int32_t Dw,
                                                       int32_t Fc, int32_t H, int32_t pW, int32_t pG, int32_t dir, float* __restrict__ d_feat,
                                                       float* __restrict__ d_wv) {
    extern __shared__ float cl_lds[];
    const int t = threadIdx.x, lane = t & 63, wid = __builtin_amdgcn_readfirstlane(t >> 6), grp = lane >> 4, col = lane & 15;
    const int I = Dw + Fc, K4 = 4 * H;
    float* wl = cl_lds;                                                         // [4H][pW]: (W_ih | W_hh)
    float* dgs = wl + K4 * pW;                                                  // [16][pG]: d_a of the step
    const float* w_ih = dir ? w_ih_r : w_ih_f;
    const float* w_hh = dir ? w_hh_r : w_hh_f;
    for (int i = t; i < K4 * pW; i += 256) {
        const int j = i / pW, n = i - j * pW;
        float v = 0.f;
        if (n < I) v = w_ih[static_cast<int64_t>(j) * I + n];
        else if (n < I + H) v = w_hh[static_cast<int64_t>(j) * H + (n - I)];
        wl[i] = v;
    }
    for (int i = t; i < 16 * pG; i += 256) dgs[i] = 0.f;
    const int u = 16 * wid + col;
    const bool active = 16 * wid < H;
    // output tiles of this wave: slot 0 = d_h of its own units, slots 1..4 = columns [16 nt, 16 nt + 16) of d_x, nt = wid + 4 (slot - 1)
    bool tv[5];
    int tc[5], tn[5];
    tv[0] = active;
    tn[0] = I + u;
    tc[0] = I + min(u, H - 1);
#pragma unroll
    for (int e = 1; e < 5; ++e) {
        const int nt = wid + 4 * (e - 1);
        tv[e] = 16 * nt < I;
        tn[e] = 16 * nt + col;
        tc[e] = min(tn[e], I - 1);
    }
    __syncthreads();
    const int64_t n_tiles = (S + 15) / 16;
    const int H5 = lstm_row_floats(H);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t s0 = tile * 16;
        float dh[4] = {0.f, 0.f, 0.f, 0.f}, dc[4] = {0.f, 0.f, 0.f, 0.f};
        float cur[4][5], nxt[4][5];
        auto slot = [&](int i, int k) {                                         // the cell of (sequence 4 grp + i, step k of the walk, unit u)
            const int tt = dir ? T - 1 - k : k;
            return lstm_saved_row(saved, static_cast<int64_t>(dir) * S + s0 + 4 * grp + i, T, tt, H5) + u;
        };
        auto fetch = [&](int k) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool ok = active && u < H && s0 + 4 * grp + i < S;
                const float* sp = slot(i, k);
#pragma unroll
                for (int q = 0; q < 5; ++q) nxt[i][q] = ok ? sp[q * H] : 0.f;
            }
        };
        fetch(T - 1);
        for (int k = T - 1; k >= 0; --k) {
            const int tt = dir ? T - 1 - k : k;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 5; ++q) cur[i][q] = nxt[i][q];
            if (k > 0) {
                fetch(k - 1);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) nxt[i][4] = 0.f;                    // c in front of the first step
            }
            if (active) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = 4 * grp + i;
                    const bool ok = u < H && s0 + m < S;
                    const float ig = cur[i][0], fg = cur[i][1], gg = cur[i][2], og = cur[i][3], ct = cur[i][4], cp = nxt[i][4];
                    float dht = dh[i];
                    if (k == T - 1 && ok) dht += g_out[(s0 + m) * (2 * H) + dir * H + u];
                    const float th = tanhf(ct);
                    const float dct = fmaf(dht * og, 1.f - th * th, dc[i]);
                    dc[i] = dct * fg;
                    const float dai = dct * gg * ig * (1.f - ig), daf = dct * cp * fg * (1.f - fg);
                    const float dag = dct * ig * (1.f - gg * gg), dao = dht * th * og * (1.f - og);
                    if (u < H) lstm_da_store(dgs + m * pG + u, H, dai, daf, dag, dao);
                    if (ok) { float* sp = slot(i, k); lstm_da_store(sp, H, dai, daf, dag, dao); sp[4 * H] = og * th; }      // h[t] where c[t] was
                }
            }
            __syncthreads();
            enc_f32x4 acc[5];
#pragma unroll
            for (int e = 0; e < 5; ++e) acc[e] = enc_f32x4{0.f, 0.f, 0.f, 0.f};
            const float* ap = dgs + col * pG + grp;
            const float* bq = wl + grp * pW;
            int kk = 0;
            for (; kk + 8 <= K4; kk += 8) {                                     // two k steps' operands are read before the first product
                const float a0 = ap[kk], a1 = ap[kk + 4];
                const float* br = bq + kk * pW;
                float b0[5], b1[5];
#pragma unroll
                for (int e = 0; e < 5; ++e)
                    if (tv[e]) { b0[e] = br[tc[e]]; b1[e] = br[4 * pW + tc[e]]; }
#pragma unroll
                for (int e = 0; e < 5; ++e)
                    if (tv[e]) acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0[e], acc[e], 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 5; ++e)
                    if (tv[e]) acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1[e], acc[e], 0, 0, 0);
            }
            if (kk < K4) {
                const float a = ap[kk];
                const float* br = bq + kk * pW;
#pragma unroll
                for (int e = 0; e < 5; ++e)
                    if (tv[e]) acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, br[tc[e]], acc[e], 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) dh[i] = acc[0][i];
#pragma unroll
            for (int e = 1; e < 5; ++e) {
                if (!tv[e] || tn[e] >= I) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t s = s0 + 4 * grp + i;
                    if (s >= S) continue;
                    float* dx = nullptr;                                        // d_x is the sum over the directions: the second launch adds
                    if (tn[e] < Dw) {
                        if (d_wv) dx = d_wv + (s * T + tt) * Dw + tn[e];
                    } else if (d_feat) {
                        dx = d_feat + (s * T + tt) * Fc + (tn[e] - Dw);
                    }
                    if (dx) *dx = dir ? *dx + acc[e][i] : acc[e][i];
                }
            }
            __syncthreads();                                                    // dgs is free for the next step
        }
    }
}

template <typename IdT>
__global__ void __launch_bounds__(256) k_ctx_lstm_wgrad(const IdT* __restrict__ words, int64_t ld_words, const float* __restrict__ table,
                                                        int32_t Vw, const float* __restrict__ feat, int64_t ld_feat,
                                                        const float* __restrict__ saved, int64_t S, int32_t T, int32_t Dw, int32_t Fc, int32_t H,
                                                        int64_t per, int32_t MT, int32_t NT, int32_t pGs, int32_t pXs,
                                                        float* __restrict__ partial) {
    extern __shared__ float cl_lds[];
    const int t = threadIdx.x, lane = t & 63, wid = __builtin_amdgcn_readfirstlane(t >> 6), grp = lane >> 4, col = lane & 15;
    const int dir = blockIdx.y, I = Dw + Fc, N = I + H + 1, K4 = 4 * H, H5 = lstm_row_floats(H), n_out = MT * NT;
    float* gs = cl_lds;                                                         // [2][16][pGs]
    float* xs = gs + 2 * 16 * pGs;                                              // [2][16][pXs]
    const int64_t sa = blockIdx.x * per, sb = min64(sa + per, S), n_rows = (sb - sa) * T, n_chunks = (n_rows + 15) / 16;
    const int lr = t >> 4, lc = t & 15;
    float gv[16], xv[21];
    auto load = [&](int64_t chunk) {                                            // row lr of the chunk: d_a and (x | h in front | 1)
        const LstmWgradRow w = lstm_wgrad_row(saved, dir, S, T, H, H5, I, sa, n_rows, chunk * 16 + lr);
        int id = 0;
        if (Dw > 0) id = lstm_id(words + w.s * ld_words + w.tt, Vw);
        const float* trow = table + static_cast<int64_t>(id) * Dw;
        const float* frow = feat + (w.s * T + w.tt) * ld_feat - Dw;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = lc + 16 * j;
            gv[j] = (w.rv && c < K4) ? w.sp[c] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 21; ++j) {
            const int c = lc + 16 * j;
            float v = 0.f;
            if (w.rv && c < N) {
                if (c < Dw) v = trow[c];
                else if (c < I) v = frow[c];
                else if (c < I + H) v = w.first ? 0.f : w.hp[c];
                else v = 1.f;
            }
            xv[j] = v;
        }
    };
    auto store = [&](int b) {
        float* gp = gs + b * 16 * pGs + lr * pGs;
        float* xp = xs + b * 16 * pXs + lr * pXs;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < MT) gp[lc + 16 * j] = gv[j];
#pragma unroll
        for (int j = 0; j < 21; ++j)
            if (j < NT) xp[lc + 16 * j] = xv[j];
    };
    enc_f32x4 acc[kClSlots];
#pragma unroll
    for (int e = 0; e < kClSlots; ++e) acc[e] = enc_f32x4{0.f, 0.f, 0.f, 0.f};
    const int mt0 = wid / NT, nt0 = wid - mt0 * NT, dq = 4 / NT, dr = 4 - dq * NT;       // tile e of this wave: index wid + 4 e = mt NT + nt
    if (n_chunks > 0) {
        load(0);
        store(0);
    }
    __syncthreads();
    for (int64_t chunk = 0; chunk < n_chunks; ++chunk) {
        const int b = static_cast<int>(chunk & 1);
        if (chunk + 1 < n_chunks) load(chunk + 1);
        const float* ga = gs + b * 16 * pGs + grp * pGs + col;
        const float* xb = xs + b * 16 * pXs + grp * pXs + col;
#pragma unroll
        for (int k0 = 0; k0 < 16; k0 += 4) {
            int mt = mt0, nt = nt0;
#pragma unroll
            for (int e = 0; e < kClSlots; ++e) {
                if (wid + 4 * e < n_out)
                    acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[k0 * pGs + 16 * mt], xb[k0 * pXs + 16 * nt], acc[e], 0, 0, 0);
                mt += dq;
                nt += dr;
                if (nt >= NT) { nt -= NT; ++mt; }
            }
        }
        if (chunk + 1 < n_chunks) store(b ^ 1);                                 // (the other buffer: its readers passed the barrier below)
        __syncthreads();
    }
    float* slab = partial + (static_cast<int64_t>(blockIdx.x) * 2 + dir) * K4 * N;      // [4H][N]
    int mt = mt0, nt = nt0;
#pragma unroll
    for (int e = 0; e < kClSlots; ++e) {
        if (wid + 4 * e < n_out) {
            const int n = 16 * nt + col;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = 16 * mt + 4 * grp + i;
                if (j < K4 && n < N) slab[static_cast<int64_t>(j) * N + n] = acc[e][i];
            }
        }
        mt += dq;
        nt += dr;
        if (nt >= NT) { nt -= NT; ++mt; }
    }
}

template <typename IdT>
int cl_launch_fwd(const void* words, int64_t ld_words, const float* table, int32_t Vw, const float* feat, int64_t ld_feat, const float* Wr,
                  int64_t S, int32_t T, int32_t Dw, int32_t Fc, int32_t H, const ClGeo& g, float* out, float* saved, hipStream_t st) {
    const size_t lds = static_cast<size_t>(g.fwd_floats) * 4;
    auto kern = &k_ctx_lstm_fwd<IdT>;
    if (!allow_lds(kern, lds)) return RECON_ERR_LAUNCH;
    const unsigned blocks = static_cast<unsigned>(min64(ceil_div64(S, 16), kClMaxWg));
    hipLaunchKernelGGL(kern, dim3(blocks, 2), dim3(256), lds, st, static_cast<const IdT*>(words), ld_words, table, Vw, feat, ld_feat, Wr, S, T, Dw,
                       Fc, H, g.Kx, g.Kh, g.pB, g.pX, g.pH, out, saved);
    return RECON_OK;
}

template <typename IdT>
int cl_launch_wgrad(const void* words, int64_t ld_words, const float* table, int32_t Vw, const float* feat, int64_t ld_feat, const float* saved,
                    int64_t S, int32_t T, int32_t Dw, int32_t Fc, int32_t H, int64_t per, int32_t G, const ClGeo& g, float* partial,
                    hipStream_t st) {
    const size_t lds = static_cast<size_t>(g.wg_floats) * 4;
    auto kern = &k_ctx_lstm_wgrad<IdT>;
    if (!allow_lds(kern, lds)) return RECON_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(G), 2), dim3(256), lds, st, static_cast<const IdT*>(words), ld_words, table, Vw, feat,
                       ld_feat, saved, S, T, Dw, Fc, H, per, g.MT, g.NT, g.pGs, g.pXs, partial);
    return RECON_OK;
}

}  // namespace
}  // namespace recon

extern "C" int recon_ctx_lstm_supported(int64_t S, int32_t T, int32_t Dw, int32_t Fc, int32_t H) {
    if (S < 1 || T < 1 || Dw < 0 || Fc < 1 || H < 1) return 0;
    if (H > recon::kClMaxH || Dw > recon::kClMaxI || Fc > recon::kClMaxI || Dw + Fc > recon::kClMaxI || T > (1 << 20)) return 0;
    const recon::ClGeo g = recon::cl_geo(Dw, Fc, H);
    if (g.fwd_floats > recon::kClLdsFloats || g.bptt_floats > recon::kClLdsFloats || g.wg_floats > recon::kClLdsFloats) return 0;
    if (g.MT * g.NT > 4 * recon::kClSlots) return 0;
    if (S > (static_cast<int64_t>(1) << 40) / (static_cast<int64_t>(T) * (5 * H > g.I ? 5 * H : g.I))) return 0;
    return 1;
}

extern "C" size_t recon_ctx_lstm_workspace_bytes(int64_t S, int32_t T, int32_t Dw, int32_t Fc, int32_t H, int32_t backward) {
    if (S <= 0 || !recon_ctx_lstm_supported(S, T, Dw, Fc, H)) return 0;
    const recon::ClGeo g = recon::cl_geo(Dw, Fc, H);
    if (!backward) return align_up(2 * (static_cast<size_t>(g.Kx + g.Kh) * g.pB + 4 * H) * 4, 256);
    int64_t per;
    int32_t G;
    recon::split_rows(S, recon::kClMaxWg, 1, &per, &G);
    return align_up(static_cast<size_t>(G) * 2 * 4 * H * g.N * 4, 256);
}

extern "C" size_t recon_ctx_lstm_saved_bytes(int64_t S, int32_t T, int32_t Dw, int32_t Fc, int32_t H) {
    if (S <= 0 || !recon_ctx_lstm_supported(S, T, Dw, Fc, H)) return 0;
    return recon::lstm_saved_bytes(S, T, H);
}

extern "C" int recon_ctx_lstm_fwd(const void* words, int32_t index_bytes, int64_t ld_words, const float* word_table, int32_t Vw, const float* feat,
                                  int64_t ld_feat, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                                  const float* w_ih_rev, const float* w_hh_rev, const float* b_ih_rev, const float* b_hh_rev, int64_t S, int32_t T,
                                  int32_t Dw, int32_t Fc, int32_t H, float* out, void* saved, void* workspace, size_t workspace_bytes,
                                  recon_stream_t stream) {
    if (S < 0 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (S == 0) return RECON_OK;
    if (!recon_ctx_lstm_supported(S, T, Dw, Fc, H)) return RECON_ERR_UNSUPPORTED;
    if (!feat || !w_ih || !w_hh || !b_ih || !b_hh || !w_ih_rev || !w_hh_rev || !b_ih_rev || !b_hh_rev || !out || !workspace || ld_feat < Fc)
        return RECON_ERR_INVALID;
    if (Dw > 0 && (!words || !word_table || Vw < 1 || ld_words < T)) return RECON_ERR_INVALID;
    if (const int rc = recon::lstm_buffer_checks(workspace, saved, workspace_bytes, recon_ctx_lstm_workspace_bytes(S, T, Dw, Fc, H, 0))) return rc;
    hipStream_t st = as_stream(stream);
    const recon::ClGeo g = recon::cl_geo(Dw, Fc, H);
    float* Wr = static_cast<float*>(workspace);
    const int64_t n_prep = 2 * (static_cast<int64_t>(g.Kx + g.Kh) * g.pB + 4 * H);
    hipLaunchKernelGGL(recon::k_ctx_lstm_prep, dim3(static_cast<unsigned>(ceil_div64(n_prep, 256))), dim3(256), 0, st, w_ih, w_hh, b_ih, b_hh, w_ih_rev,
                       w_hh_rev, b_ih_rev, b_hh_rev, g.I, H, g.Kx, g.Kh, g.pB, Wr);
    RECON_CHECK_LAUNCH();
    const int rc = recon::dispatch_ids(index_bytes, [&](auto id) {
        return recon::cl_launch_fwd<typename decltype(id)::type>(words, ld_words, word_table, Vw, feat, ld_feat, Wr, S, T, Dw, Fc, H, g, out,
                                                                 static_cast<float*>(saved), st);
    });
    if (rc != RECON_OK) return rc;
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_ctx_lstm_bwd(const void* words, int32_t index_bytes, int64_t ld_words, const float* word_table, int32_t Vw, const float* feat,
                                  int64_t ld_feat, const float* w_ih, const float* w_hh, const float* w_ih_rev, const float* w_hh_rev,
                                  const float* g_out, void* saved, int64_t S, int32_t T, int32_t Dw, int32_t Fc, int32_t H, float* d_feat,
                                  float* d_word_vec, float* g_w_ih, float* g_w_hh, float* g_b_ih, float* g_b_hh, float* g_w_ih_rev,
                                  float* g_w_hh_rev, float* g_b_ih_rev, float* g_b_hh_rev, void* workspace, size_t workspace_bytes,
                                  recon_stream_t stream) {
    if (S < 0 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (!recon_ctx_lstm_supported(S > 0 ? S : 1, T, Dw, Fc, H)) return RECON_ERR_UNSUPPORTED;
    if (!g_w_ih || !g_w_hh || !g_b_ih || !g_b_hh || !g_w_ih_rev || !g_w_hh_rev || !g_b_ih_rev || !g_b_hh_rev) return RECON_ERR_INVALID;
    hipStream_t st = as_stream(stream);
    const int32_t I = Dw + Fc;
    if (S == 0) return recon::lstm_zero_param_grads(g_w_ih, g_w_hh, g_b_ih, g_b_hh, g_w_ih_rev, g_w_hh_rev, g_b_ih_rev, g_b_hh_rev, I, H, st);
    if (!feat || !w_ih || !w_hh || !w_ih_rev || !w_hh_rev || !g_out || !saved || !workspace || ld_feat < Fc) return RECON_ERR_INVALID;
    if (Dw > 0 && (!words || !word_table || Vw < 1 || ld_words < T)) return RECON_ERR_INVALID;
    if (const int rc = recon::lstm_buffer_checks(workspace, saved, workspace_bytes, recon_ctx_lstm_workspace_bytes(S, T, Dw, Fc, H, 1))) return rc;
    const recon::ClGeo g = recon::cl_geo(Dw, Fc, H);
    {
        const size_t lds = static_cast<size_t>(g.bptt_floats) * 4;
        if (!recon::allow_lds(&recon::k_ctx_lstm_bptt, lds)) return RECON_ERR_LAUNCH;
        const unsigned blocks = static_cast<unsigned>(recon::min64(ceil_div64(S, 16), 2 * recon::kClMaxWg));
        for (int dir = 0; dir < 2; ++dir) {                                     // one launch per direction: the second adds its d_x to the first's
            hipLaunchKernelGGL(recon::k_ctx_lstm_bptt, dim3(blocks), dim3(256), lds, st, w_ih, w_hh, w_ih_rev, w_hh_rev, g_out,
                               static_cast<float*>(saved), S, T, Dw, Fc, H, g.pW, g.pG, dir, d_feat, Dw > 0 ? d_word_vec : nullptr);
            RECON_CHECK_LAUNCH();
        }
    }
    int64_t per;
    int32_t G;
    recon::split_rows(S, recon::kClMaxWg, 1, &per, &G);
    float* partial = static_cast<float*>(workspace);
    const int rc = recon::dispatch_ids(index_bytes, [&](auto id) {
        return recon::cl_launch_wgrad<typename decltype(id)::type>(words, ld_words, word_table, Vw, feat, ld_feat, static_cast<const float*>(saved), S, T, Dw, Fc,
                                                                   H, per, G, g, partial, st);
    });
    if (rc != RECON_OK) return rc;
    RECON_CHECK_LAUNCH();
    hipLaunchKernelGGL(recon::k_lstm_reduce, dim3(static_cast<unsigned>(ceil_div64(static_cast<int64_t>(2) * 4 * H * g.N, 256))), dim3(256), 0, st,
                       partial, G, I, H, 0, g_w_ih, g_w_hh, g_b_ih, g_b_hh, g_w_ih_rev, g_w_hh_rev, g_b_ih_rev, g_b_hh_rev, static_cast<float*>(nullptr));
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}
