// What the two bidirectional LSTM ops (ctx_lstm.hip, sent_lstm.hip) share: the forward cell, the saved-state contract between their five kernels
// each, the slab reduce and the host checks.  Saved state: 5 H floats (i, f, g, o, c[t]) per (direction, sequence, step), H apart; the BPTT pass
// leaves d_a where the gates were and h[t] where c[t] was (`sp[4 * H] = o tanh(c[t])` in both files), which the weight-gradient pass reads.
// "Once" in a weaker sense than one would like: the callers form ds = dir S + s and the row length themselves and the BPTT cell formulas stay in
// both files, because the device code is kept instruction for instruction.  Every kernel but the reduce stays in its file.
#pragma once
#include <math.h>
#include "ctx_enc_common.h"

namespace recon {

inline int lstm_pitch(int n, int mod32) { int p = n; while (p % 32 != mod32) ++p; return p; }
inline size_t lstm_saved_bytes(int64_t S, int32_t T, int32_t H) { return static_cast<size_t>(2) * S * T * 5 * H * 4; }
__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
// an id clamped into its table: an id outside [0, V) is the caller's error, never an access outside
template <typename IdT>
__device__ __forceinline__ int lstm_id(const IdT* p, int V) {
    const int64_t v = static_cast<int64_t>(*p);
    return static_cast<int>(v < 0 ? 0 : (v >= V ? V - 1 : v));
}
// the floats of a cell row, and the row of (dir, s, tt): ds = dir S + s, the sequence's index over both directions, H5 = lstm_row_floats(H)
__device__ __forceinline__ int lstm_row_floats(int32_t H) { return 5 * H; }
template <typename F>
__device__ __forceinline__ F* lstm_saved_row(F* saved, int64_t ds, int32_t T, int tt, int H5) { return saved + (ds * T + tt) * H5; }

// gate products a_*, the four biases b and c[t'] -> the gates, c[t] in place, h[t]
__device__ __forceinline__ float lstm_cell_fwd(float a_i, float a_f, float a_g, float a_o, const float (&b)[4], float& c, float& i, float& f, float& g,
                                               float& o) {
    i = lstm_sigmoid(a_i + b[0]), f = lstm_sigmoid(a_f + b[1]);
    g = tanhf(a_g + b[2]), o = lstm_sigmoid(a_o + b[3]);
    c = fmaf(f, c, i * g);
    return o * tanhf(c);
}
__device__ __forceinline__ void lstm_cell_store(float* sp, int32_t H, float i, float f, float g, float o, float c) {
    sp[0] = i; sp[H] = f; sp[2 * H] = g; sp[3 * H] = o; sp[4 * H] = c;
}
// the BPTT pass: d_a into the LDS tile of the step or over the gates of a saved row
__device__ __forceinline__ void lstm_da_store(float* p, int32_t H, float d_ai, float d_af, float d_ag, float d_ao) {
    p[0] = d_ai; p[H] = d_af; p[2 * H] = d_ag; p[3 * H] = d_ao;
}

// row r of a weight-gradient workgroup's n_rows = (its sequences from sa on) x T: the cell row sp, whether it is its walk's first step, and hp
// with hp[c] = h of the step in front for the columns I <= c < I + H of (x | h | ...): that h lies where its c was
struct LstmWgradRow { bool rv, first; int64_t s; int tt; const float* sp; const float* hp; };
__device__ __forceinline__ LstmWgradRow lstm_wgrad_row(const float* saved, int dir, int64_t S, int32_t T, int32_t H, int H5, int I, int64_t sa,
                                                       int64_t n_rows, int64_t r) {
    LstmWgradRow w;
    w.rv = r < n_rows;
    w.s = w.rv ? sa + r / T : sa;
    w.tt = w.rv ? static_cast<int>(r % T) : 0;
    w.sp = lstm_saved_row(saved, static_cast<int64_t>(dir) * S + w.s, T, w.tt, H5);
    w.first = dir ? w.tt == T - 1 : w.tt == 0;
    w.hp = w.sp + (dir ? H5 : -H5) + 4 * H - I;
    return w;
}

namespace {
// the G slabs added in slab order; cell (dir, j, n): n < I -> g_w_ih[j][n], n < I + H -> g_w_hh[j][n - I], n = I + H -> both bias
// gradients, behind it the pair LSTM's class sum D[dir][j][n - I - H - 1] (the line LSTM: Vp = 0, cls = nullptr)
__global__ void __launch_bounds__(256) k_lstm_reduce(const float* __restrict__ partial, int32_t G, int32_t I, int32_t H, int32_t Vp,
                                                     float* __restrict__ g_w_ih_f, float* __restrict__ g_w_hh_f, float* __restrict__ g_b_ih_f,
                                                     float* __restrict__ g_b_hh_f, float* __restrict__ g_w_ih_r, float* __restrict__ g_w_hh_r,
                                                     float* __restrict__ g_b_ih_r, float* __restrict__ g_b_hh_r, float* __restrict__ cls) {
    const int N = I + H + 1 + Vp, per = 4 * H * N;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * per) return;
    float sum = 0.f;
#pragma unroll 8
    for (int g = 0; g < G; ++g) sum += partial[static_cast<int64_t>(g) * 2 * per + i];
    const int dir = i / per, r = i - dir * per, j = r / N, n = r - j * N;
    if (n < I) {
        (dir ? g_w_ih_r : g_w_ih_f)[static_cast<int64_t>(j) * I + n] = sum;
    } else if (n < I + H) {
        (dir ? g_w_hh_r : g_w_hh_f)[static_cast<int64_t>(j) * H + (n - I)] = sum;
    } else if (n == I + H) {
        (dir ? g_b_ih_r : g_b_ih_f)[j] = sum;
        (dir ? g_b_hh_r : g_b_hh_f)[j] = sum;
    } else {
        cls[(static_cast<int64_t>(dir) * 4 * H + j) * Vp + (n - I - H - 1)] = sum;
    }
}
}  // namespace

// the eight parameter gradients of an empty batch, zeroed in the order both entries always had
inline int lstm_zero_param_grads(float* g_w_ih, float* g_w_hh, float* g_b_ih, float* g_b_hh, float* g_w_ih_rev, float* g_w_hh_rev, float* g_b_ih_rev,
                                 float* g_b_hh_rev, int32_t I, int32_t H, hipStream_t st) {
    const size_t n_ih = static_cast<size_t>(4) * H * I, n_hh = static_cast<size_t>(4) * H * H, n_b = static_cast<size_t>(4) * H;
    return zero_fill({{g_w_ih, n_ih}, {g_w_ih_rev, n_ih}, {g_w_hh, n_hh}, {g_w_hh_rev, n_hh}, {g_b_ih, n_b}, {g_b_ih_rev, n_b}, {g_b_hh, n_b},
                      {g_b_hh_rev, n_b}}, st);
}
// workspace and saved state aligned, the workspace of `need` bytes
inline int lstm_buffer_checks(const void* workspace, const void* saved, size_t workspace_bytes, size_t need) {
    if (reinterpret_cast<uintptr_t>(workspace) % 16 || reinterpret_cast<uintptr_t>(saved) % 16) return RECON_ERR_INVALID;
    return workspace_bytes < need ? RECON_ERR_WORKSPACE : RECON_OK;
}
// (32-row tile, two unit blocks per wave) -> the <RT, UB> instance of a launch: f(IntTag<RT>, IntTag<UB>) names its argument list once
template <int N> using IntTag = std::integral_constant<int, N>;
template <typename F>
int dispatch_tile(bool wide, bool two, F&& f) {
    if (wide) return two ? f(IntTag<2>{}, IntTag<2>{}) : f(IntTag<2>{}, IntTag<1>{});
    return two ? f(IntTag<1>{}, IntTag<2>{}) : f(IntTag<1>{}, IntTag<1>{});
}

}  // namespace recon
