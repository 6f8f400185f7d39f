// The sentence encoder's pair LSTM (models/models.py:160-184): one layer, two directions, batch_first, S = B C sequences of exactly T
// steps (sequence s = b C + c is sentence b seen from entity pair c), only the two final hidden states kept:
//     x[s][t]   = (word_table[sentence[b][t]] * keep[s][t] | pos_table[markers[s][t]])       (I = Dw + P; never written)
//     a[s][t]   = W_ih x[s][t] + b_ih + W_hh h[s][t'] + b_hh,  t' the step before t in the direction's walk, h = c = 0 in front of it
//     i, f, o   = sigmoid(a[0:H], a[H:2H], a[3H:4H]),  g = tanh(a[2H:3H]),  c[t] = f c[t'] + i g,  h[t] = o tanh(c[t])
//     out[s]    = (h_fwd after t = T - 1 | h_rev after t = 0)
// Everything is fp32 on v_mfma_f32_16x16x4_f32; no floating-point atomics, every sum has one order.  H goes up to 256, so one direction's
// weights (1.27 MB at I = 53) do not fit a CU's LDS: every B fragment is used by one wave only and goes from global memory / L2 straight
// into registers, 16 bytes per lane, from a layout k_sent_lstm_prep_* writes once per call.  Every workgroup is independent: it owns one
// tile of sequences of one direction for all T steps.
//
// B-operand order ("fragment order"): a 16 x 16 output tile's operand for 16 values of k is 64 lanes x 4 floats, lane (grp, col) holding
//   k = 16 k16 + 4 grp + i (i = 0..3) of column col; MFMA i of the four takes element i of both the A and the B vector.  The A operand
//   comes out of LDS as one 16-byte read per lane in the same k order.
// k_sent_lstm_prep_fwd: Wr[dir][unit block nb][gate q][k16][lane][4] over the rows (W_ih^T, zeros up to Kx = 4 ceil(I / 4); W_hh^T; zeros up
//   to a multiple of 16), followed by b_ih + b_hh.  k_sent_lstm_prep_bwd: W_hh as Whr[dir][nb][k16][lane][4] with k the gate row.
// k_sent_lstm_fwd<RT, UB>: 8 waves, a tile of 16 RT sequences.  The rows (x[t] | h[t']) lie in LDS, two buffers: a step reads one and
//   writes h[t] and x[t + 1] into the other, one barrier per step.  Wave w owns the hidden units [16 UB w, 16 UB (w + 1)) and the four gate
//   tiles of each: i, f, g, o of a cell meet in one lane, c never leaves registers.  With `saved` it writes (i, f, g, o, c) of every step.
// k_sent_lstm_bptt<RT, UB>: per tile the steps backwards; d_h and d_c stay in registers in the forward's lane layout, the step's d_a goes
//   through LDS as the A operand against W_hh (K = 4H, N = H).  It leaves d_a where the gates were and h[t] where c[t] was.  No d_x.
// k_sent_lstm_wgrad: d_a^T (x | h[t'] | 1 | onehot(marker)) over the S T rows; grid (row groups) x (blocks of 128 gate rows) x direction,
//   wave w owns gate rows [16 w, 16 w + 16) of the block and every column tile; 16 rows at a time through LDS.  Each workgroup writes its
//   slab; k_lstm_reduce (lstm_common.h) adds the slabs in group order and scatters into the eight gradients and the class sums
//   D[dir][j][v] = sum over the rows with marker v of d_a[j]; k_sent_lstm_dpos: d_pos[v] = sum_dir D[dir][:, v]^T W_ih[:, Dw:].
#include "lstm_common.h"

namespace recon {
namespace {

constexpr int kSlThreads = 512;                // eight waves
constexpr int kSlMaxH = 256;                   // eight waves x two 16-unit blocks
constexpr int kSlMaxI = 128;                   // Dw + P
constexpr int kSlMaxVp = 16;                   // rows of pos_table (one-hot columns of the weight-gradient pass)
constexpr int kSlWideFrom = 2048;              // above this many sequences a tile is 32 rows, else 16
constexpr int kSlMaxGroups = 32;               // row groups of the weight-gradient pass
constexpr int kSlGateRows = 128;               // gate rows per workgroup of the weight-gradient pass
constexpr int kSlSlots = 28;                   // column tiles of (x | h | 1 | onehot), in fours: ceil((128 + 256 + 1 + 16) / 16) = 26 -> 28

struct SlGeo {
    int32_t I, Kx, K16, pA, NB, UB, NBp;       // forward
    int32_t K16b, pG;                          // BPTT
    int32_t N, NT, pGs, pXs, JB;               // weight gradient
    int64_t wr_dir, whr_dir;                   // floats per direction of the two operand layouts
};
inline SlGeo sl_geo(int32_t Dw, int32_t P, int32_t H, int32_t Vp) {
    SlGeo g;
    g.I = Dw + P;
    g.Kx = (g.I + 3) / 4 * 4;
    g.K16 = (g.Kx + H + 15) / 16;
    g.pA = 16 * g.K16 + 4;                      // rows 16 bytes apart modulo 64: the 16-byte reads of 8 lanes cover the 32 banks
    g.NB = (H + 15) / 16;
    g.UB = g.NB > 8 ? 2 : 1;
    g.NBp = (g.NB + g.UB - 1) / g.UB * g.UB;
    g.K16b = (4 * H + 15) / 16;
    g.pG = 16 * g.K16b + 4;
    g.N = g.I + H + 1 + Vp;
    g.NT = (g.N + 15) / 16;
    g.pGs = lstm_pitch(kSlGateRows, 16);
    g.pXs = lstm_pitch(16 * ((g.NT + 3) / 4 * 4), 16);      // the products take the column tiles four at a time: zeros behind NT
    g.JB = (4 * H + kSlGateRows - 1) / kSlGateRows;
    g.wr_dir = static_cast<int64_t>(g.NBp) * 4 * g.K16 * 256 + 4 * H;
    g.whr_dir = static_cast<int64_t>(g.NBp) * g.K16b * 256;
    return g;
}
inline int sl_row_tiles(int64_t S) { return S > kSlWideFrom ? 2 : 1; }

// An address (or index) the compiler must form before the load that uses it: a load whose address is a select would otherwise be sunk into
// per-column branches, and loads in branches wait for one another (one memory latency each instead of one for all of them).
template <typename V>
__device__ __forceinline__ void sl_opaque(V& v) { asm volatile("" : "+v"(v)); }
// (behind the asm the compiler no longer knows the pointer is global and would issue a flat load, which every LDS wait waits for)
__device__ __forceinline__ float sl_global(const float* p) { return *(const __attribute__((address_space(1))) float*)p; }

__global__ void __launch_bounds__(256) k_sent_lstm_prep_fwd(const float* __restrict__ w_ih_f, const float* __restrict__ w_hh_f,
                                                            const float* __restrict__ b_ih_f, const float* __restrict__ b_hh_f,
                                                            const float* __restrict__ w_ih_r, const float* __restrict__ w_hh_r,
                                                            const float* __restrict__ b_ih_r, const float* __restrict__ b_hh_r, int32_t I, int32_t H,
                                                            int32_t Kx, int32_t K16, int64_t per, float* __restrict__ Wr) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= 2 * per) return;
    const int dir = static_cast<int>(i / per);
    const int64_t r = i - dir * per;
    const float* w_ih = dir ? w_ih_r : w_ih_f;
    const float* w_hh = dir ? w_hh_r : w_hh_f;
    float v = 0.f;
    if (r >= per - 4 * H) {
        const int j = static_cast<int>(r - (per - 4 * H));
        v = (dir ? b_ih_r : b_ih_f)[j] + (dir ? b_hh_r : b_hh_f)[j];
    } else {
        const int ii = static_cast<int>(r & 3), lane = static_cast<int>((r >> 2) & 63);
        const int64_t frag = r >> 8;
        const int k16 = static_cast<int>(frag % K16), tile = static_cast<int>(frag / K16), nb = tile >> 2, q = tile & 3;
        const int kk = 16 * k16 + 4 * (lane >> 4) + ii, u = 16 * nb + (lane & 15);
        if (u < H) {
            const int64_t n = static_cast<int64_t>(q) * H + u;
            if (kk < I) v = w_ih[n * I + kk];
            else if (kk >= Kx && kk - Kx < H) v = w_hh[n * H + (kk - Kx)];
        }
    }
    Wr[i] = v;
}

__global__ void __launch_bounds__(256) k_sent_lstm_prep_bwd(const float* __restrict__ w_hh_f, const float* __restrict__ w_hh_r, int32_t H,
                                                            int32_t K16b, int64_t per, float* __restrict__ Whr) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= 2 * per) return;
    const int dir = static_cast<int>(i / per);
    const int64_t r = i - dir * per;
    const int ii = static_cast<int>(r & 3), lane = static_cast<int>((r >> 2) & 63);
    const int64_t frag = r >> 8;
    const int k16 = static_cast<int>(frag % K16b), nb = static_cast<int>(frag / K16b);
    const int j = 16 * k16 + 4 * (lane >> 4) + ii, u = 16 * nb + (lane & 15);
    float v = 0.f;
    if (j < 4 * H && u < H) v = (dir ? w_hh_r : w_hh_f)[static_cast<int64_t>(j) * H + u];
    Whr[i] = v;
}

template <typename IdT, int RT, int UB>
__global__ void __launch_bounds__(kSlThreads) k_sent_lstm_fwd(const IdT* __restrict__ sentence, int64_t ld_sent, const IdT* __restrict__ markers,
                                                              int64_t ld_mark, const float* __restrict__ table, int32_t Vw,
                                                              const float* __restrict__ pos, int32_t Vp, const int32_t* __restrict__ bits,
                                                              float scale, const float* __restrict__ Wr, int64_t wr_dir, int64_t S, int32_t C,
                                                              int32_t T, int32_t Dw, int32_t P, int32_t H, int32_t Kx, int32_t K16, int32_t pA,
                                                              float* __restrict__ out, float* __restrict__ saved) {
    extern __shared__ float sl_lds[];
    constexpr int M = 16 * RT, TPR = kSlThreads / M, NJ = kSlMaxI / TPR;
    const int t = threadIdx.x, lane = t & 63, wid = __builtin_amdgcn_readfirstlane(t >> 6), grp = lane >> 4, col = lane & 15;
    const int dir = blockIdx.y, I = Dw + P, KW = (Dw + 31) >> 5;
    float* As = sl_lds;                                                         // [2][M][pA]: (x | h in front | zeros)
    for (int i = t; i < 2 * M * pA; i += kSlThreads) As[i] = 0.f;               // h in front of the first step; the tails stay zero for good
    const float* wdir = Wr + dir * wr_dir;
    const int nb0 = wid * UB;
    const bool active = 16 * nb0 < H;
    float bias[UB][4];
#pragma unroll
    for (int ub = 0; ub < UB; ++ub)
#pragma unroll
        for (int q = 0; q < 4; ++q) bias[ub][q] = wdir[wr_dir - 4 * H + q * H + min(16 * (nb0 + ub) + col, H - 1)];
    const int lr = t / TPR, lc = t - lr * TPR;
    const int64_t s0 = static_cast<int64_t>(blockIdx.x) * M, srow = s0 + lr;
    const bool sv = srow < S;
    const int64_t b = sv ? srow / C : 0;
    // The next step's row: load_x only issues loads (every address valid whatever the column, no branch between them, so that they are
    // in flight together under the step's products); store_x applies the keep bits and writes the row.
    float xv[NJ];
    int32_t wbw[4] = {0, 0, 0, 0};
    auto load_x = [&](int tt) {                                                 // row lr of step tt: columns lc, lc + TPR, ...
        int wi = 0, mk = 0;
        if (sv) {
            wi = lstm_id(sentence + b * ld_sent + tt, Vw);
            mk = lstm_id(markers + srow * ld_mark + tt, Vp);
        }
        const float* trow = table + static_cast<int64_t>(wi) * Dw;
        const float* prow = pos + static_cast<int64_t>(mk) * P - Dw;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lc + TPR * j;
            const float* src = c < Dw ? trow + c : (c < I ? prow + c : trow);
            sl_opaque(src);
            xv[j] = sl_global(src);
        }
        if (bits) {
            const int32_t* brow = bits + ((sv ? srow : 0) * T + tt) * KW;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int at = q < KW ? q : 0;
                sl_opaque(at);
                wbw[q] = brow[at];
            }
        }
    };
    auto store_x = [&](float* buf) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lc + TPR * j;
            float v = xv[j];
            if (bits && c < Dw) v = ((wbw[(TPR * j) >> 5] >> (c & 31)) & 1) ? v * scale : 0.f;     // (lc < TPR <= 32: c >> 5 is a constant)
            if (c < I) buf[lr * pA + c] = sv ? v : 0.f;
        }
    };
    load_x(dir ? T - 1 : 0);
    __syncthreads();                                                            // the zero fill is complete
    store_x(As);
    float c[RT][UB][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ub = 0; ub < UB; ++ub)
#pragma unroll
            for (int i = 0; i < 4; ++i) c[rt][ub][i] = 0.f;
    __syncthreads();
    const float* bp = wdir + static_cast<int64_t>(nb0) * 4 * K16 * 256 + lane * 4;
    for (int k = 0; k < T; ++k) {
        const int tt = dir ? T - 1 - k : k;
        if (k + 1 < T) load_x(dir ? tt - 1 : tt + 1);                           // flies during this step's products
        const float* cur = As + (k & 1) * M * pA;
        float* nxt = As + ((k & 1) ^ 1) * M * pA;
        if (active) {
            enc_f32x4 acc[RT][UB][4];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ub = 0; ub < UB; ++ub)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[rt][ub][q] = enc_f32x4{0.f, 0.f, 0.f, 0.f};
            const float* ap = cur + col * pA + 4 * grp;
            enc_f32x4 bc[UB][4], bn[UB][4];
#pragma unroll
            for (int ub = 0; ub < UB; ++ub)
#pragma unroll
                for (int q = 0; q < 4; ++q) bc[ub][q] = *reinterpret_cast<const enc_f32x4*>(bp + static_cast<int64_t>(ub * 4 + q) * K16 * 256);
            for (int k16 = 0; k16 < K16; ++k16) {
                const int kn = k16 + 1 < K16 ? k16 + 1 : k16;                   // the next fragments are on their way under this one's products
#pragma unroll
                for (int ub = 0; ub < UB; ++ub)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        bn[ub][q] = *reinterpret_cast<const enc_f32x4*>(bp + (static_cast<int64_t>(ub * 4 + q) * K16 + kn) * 256);
                enc_f32x4 a[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) a[rt] = *reinterpret_cast<const enc_f32x4*>(ap + rt * 16 * pA + 16 * k16);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int ub = 0; ub < UB; ++ub)
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                acc[rt][ub][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][i], bc[ub][q][i], acc[rt][ub][q], 0, 0, 0);
#pragma unroll
                for (int ub = 0; ub < UB; ++ub)
#pragma unroll
                    for (int q = 0; q < 4; ++q) bc[ub][q] = bn[ub][q];
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ub = 0; ub < UB; ++ub) {
                    const int u = 16 * (nb0 + ub) + col;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int m = 16 * rt + 4 * grp + i;
                        float ig, fg, gg, og;
                        const float h = lstm_cell_fwd(acc[rt][ub][0][i], acc[rt][ub][1][i], acc[rt][ub][2][i], acc[rt][ub][3][i], bias[ub], c[rt][ub][i],
                                                      ig, fg, gg, og);
                        if (u < H) {
                            nxt[m * pA + Kx + u] = h;
                            if (s0 + m < S) {
                                if (saved) {
                                    float* sp = lstm_saved_row(saved, static_cast<int64_t>(dir) * S + s0 + m, T, tt, lstm_row_floats(H)) + u;
                                    lstm_cell_store(sp, H, ig, fg, gg, og, c[rt][ub][i]);
                                }
                                if (k == T - 1) out[(s0 + m) * (2 * H) + dir * H + u] = h;
                            }
                        }
                    }
                }
        }
        if (k + 1 < T) store_x(nxt);
        __syncthreads();                                                        // nxt is complete; every wave is done with cur
    }
}

template <int RT, int UB>
__global__ void __launch_bounds__(kSlThreads) k_sent_lstm_bptt(const float* __restrict__ Whr, int64_t whr_dir, const float* __restrict__ g_out,
                                                               float* __restrict__ saved, int64_t S, int32_t T, int32_t H, int32_t K16b,
                                                               int32_t pG) {
    extern __shared__ float sl_lds[];
    constexpr int M = 16 * RT;
    const int t = threadIdx.x, lane = t & 63, wid = __builtin_amdgcn_readfirstlane(t >> 6), grp = lane >> 4, col = lane & 15;
    const int dir = blockIdx.y, H5 = lstm_row_floats(H);
    float* dgs = sl_lds;                                                        // [M][pG]: d_a of the step
    for (int i = t; i < M * pG; i += kSlThreads) dgs[i] = 0.f;                  // (the tail behind 4H stays zero)
    const int nb0 = wid * UB;
    const bool active = 16 * nb0 < H;
    const int64_t s0 = static_cast<int64_t>(blockIdx.x) * M;
    const float* bp = Whr + dir * whr_dir + static_cast<int64_t>(nb0) * K16b * 256 + lane * 4;
    float dh[RT][UB][4], dc[RT][UB][4], ct[RT][UB][4];
    auto slot = [&](int m, int k) {                                             // the cell row of (sequence s0 + m, step k of the walk)
        const int tt = dir ? T - 1 - k : k;
        return lstm_saved_row(saved, static_cast<int64_t>(dir) * S + s0 + m, T, tt, H5);
    };
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ub = 0; ub < UB; ++ub) {
            const int u = 16 * (nb0 + ub) + col;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = 16 * rt + 4 * grp + i;
                dh[rt][ub][i] = 0.f;
                dc[rt][ub][i] = 0.f;
                ct[rt][ub][i] = (active && u < H && s0 + m < S) ? slot(m, T - 1)[4 * H + u] : 0.f;
            }
        }
    __syncthreads();
    for (int k = T - 1; k >= 0; --k) {
        if (active) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ub = 0; ub < UB; ++ub) {
                    const int u = 16 * (nb0 + ub) + col;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int m = 16 * rt + 4 * grp + i;
                        const bool ok = u < H && s0 + m < S;
                        float ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, cp = 0.f, go = 0.f;
                        float* sp = slot(m, k) + u;
                        if (ok) {
                            ig = sp[0]; fg = sp[H]; gg = sp[2 * H]; og = sp[3 * H];
                            if (k > 0) cp = slot(m, k - 1)[4 * H + u];
                            if (k == T - 1) go = g_out[(s0 + m) * (2 * H) + dir * H + u];
                        }
                        const float dht = dh[rt][ub][i] + go;
                        const float th = tanhf(ct[rt][ub][i]);
                        const float dct = fmaf(dht * og, 1.f - th * th, dc[rt][ub][i]);
                        dc[rt][ub][i] = dct * fg;
                        const float dai = dct * gg * ig * (1.f - ig), daf = dct * cp * fg * (1.f - fg);
                        const float dag = dct * ig * (1.f - gg * gg), dao = dht * th * og * (1.f - og);
                        ct[rt][ub][i] = cp;
                        if (u < H) { float* dp = dgs + m * pG + u; lstm_da_store(dp, H, dai, daf, dag, dao); }
                        if (ok) { lstm_da_store(sp, H, dai, daf, dag, dao); sp[4 * H] = og * th; }     // h[t] where c[t] was
                    }
                }
        }
        __syncthreads();
        if (active && k > 0) {
            enc_f32x4 acc[RT][UB];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ub = 0; ub < UB; ++ub) acc[rt][ub] = enc_f32x4{0.f, 0.f, 0.f, 0.f};
            const float* ap = dgs + col * pG + 4 * grp;
            enc_f32x4 bc[UB], bn[UB];
#pragma unroll
            for (int ub = 0; ub < UB; ++ub) bc[ub] = *reinterpret_cast<const enc_f32x4*>(bp + static_cast<int64_t>(ub) * K16b * 256);
            for (int k16 = 0; k16 < K16b; ++k16) {
                const int kn = k16 + 1 < K16b ? k16 + 1 : k16;
#pragma unroll
                for (int ub = 0; ub < UB; ++ub) bn[ub] = *reinterpret_cast<const enc_f32x4*>(bp + (static_cast<int64_t>(ub) * K16b + kn) * 256);
                enc_f32x4 a[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) a[rt] = *reinterpret_cast<const enc_f32x4*>(ap + rt * 16 * pG + 16 * k16);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int ub = 0; ub < UB; ++ub) acc[rt][ub] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][i], bc[ub][i], acc[rt][ub], 0, 0, 0);
#pragma unroll
                for (int ub = 0; ub < UB; ++ub) bc[ub] = bn[ub];
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ub = 0; ub < UB; ++ub)
#pragma unroll
                    for (int i = 0; i < 4; ++i) dh[rt][ub][i] = acc[rt][ub][i];
        }
        __syncthreads();                                                        // dgs is free for the next step
    }
}

template <typename IdT>
__global__ void __launch_bounds__(kSlThreads) k_sent_lstm_wgrad(const IdT* __restrict__ sentence, int64_t ld_sent, const IdT* __restrict__ markers,
                                                                int64_t ld_mark, const float* __restrict__ table, int32_t Vw,
                                                                const float* __restrict__ pos, int32_t Vp, const int32_t* __restrict__ bits,
                                                                float scale, const float* __restrict__ saved, int64_t S, int32_t C, int32_t T,
                                                                int32_t Dw, int32_t P, int32_t H, int64_t per, int32_t NT, int32_t pGs,
                                                                int32_t pXs, float* __restrict__ partial) {
    extern __shared__ float sl_lds[];
    const int t = threadIdx.x, lane = t & 63, wid = __builtin_amdgcn_readfirstlane(t >> 6), grp = lane >> 4, col = lane & 15;
    const int dir = blockIdx.z, j0 = blockIdx.y * kSlGateRows, I = Dw + P, N = I + H + 1 + Vp, K4 = 4 * H, H5 = lstm_row_floats(H), KW = (Dw + 31) >> 5;
    float* gs = sl_lds;                                                         // [2][16][pGs]
    float* xs = gs + 2 * 16 * pGs;                                              // [2][16][pXs]
    const int NT4 = (NT + 3) / 4 * 4;
    const int64_t sa = blockIdx.x * per, sb = min64(sa + per, S), n_rows = (sb - sa) * T, n_chunks = (n_rows + 15) / 16;
    const int lr = t >> 5, lc = t & 31;
    constexpr int NG = kSlGateRows / 32, NX = kSlSlots / 2;
    // load only issues loads (every address valid whatever the column and the row, no branch between them, so that they are in flight
    // together under the chunk's products); store applies the keep bits, the zeros, the ones and the one-hot columns and writes the rows.
    float gv[NG], xv[NX];
    int32_t wbw[4] = {0, 0, 0, 0};
    int row_mk = 0;
    bool row_rv = false, row_hv = false;
    auto load = [&](int64_t chunk) {                                            // row lr of the chunk: d_a and (x | h in front | 1 | onehot)
        const LstmWgradRow w = lstm_wgrad_row(saved, dir, S, T, H, H5, I, sa, n_rows, chunk * 16 + lr);
        const int wi = lstm_id(sentence + (w.s / C) * ld_sent + w.tt, Vw);
        const int mk = lstm_id(markers + w.s * ld_mark + w.tt, Vp);
        const float* trow = table + static_cast<int64_t>(wi) * Dw;
        const float* prow = pos + static_cast<int64_t>(mk) * P - Dw;
        row_mk = mk;
        row_rv = w.rv;
        row_hv = w.rv && !w.first;
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int c = j0 + lc + 32 * j;
            int at = c < K4 ? c : 0;
            sl_opaque(at);
            gv[j] = w.sp[at];
        }
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            const int c = lc + 32 * j;
            const float* src = c < Dw ? trow + c : (c < I ? prow + c : ((c < I + H && row_hv) ? w.hp + c : trow));
            sl_opaque(src);
            xv[j] = sl_global(src);
        }
        if (bits) {
            const int32_t* brow = bits + (w.s * T + w.tt) * KW;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int at = q < KW ? q : 0;
                sl_opaque(at);
                wbw[q] = brow[at];
            }
        }
    };
    auto store = [&](int b) {
        float* gp = gs + b * 16 * pGs + lr * pGs;
        float* xp = xs + b * 16 * pXs + lr * pXs;
#pragma unroll
        for (int j = 0; j < NG; ++j) gp[lc + 32 * j] = (row_rv && j0 + lc + 32 * j < K4) ? gv[j] : 0.f;
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            const int c = lc + 32 * j;
            float v = xv[j];
            if (bits && c < Dw) v = ((wbw[j & 3] >> lc) & 1) ? v * scale : 0.f;                  // (lc < 32: c >> 5 = j, and Dw <= 128)
            if (c >= I && c < I + H && !row_hv) v = 0.f;
            if (c == I + H) v = 1.f;
            if (c > I + H) v = (c - (I + H + 1) == row_mk) ? 1.f : 0.f;
            if (lc + 32 * j < 16 * NT4) xp[lc + 32 * j] = (row_rv && c < N) ? v : 0.f;
        }
    };
    enc_f32x4 acc[kSlSlots];
#pragma unroll
    for (int e = 0; e < kSlSlots; ++e) acc[e] = enc_f32x4{0.f, 0.f, 0.f, 0.f};
    const bool active = j0 + 16 * wid < K4;
    if (n_chunks > 0) {
        load(0);
        store(0);
    }
    __syncthreads();
    for (int64_t chunk = 0; chunk < n_chunks; ++chunk) {
        const int b = static_cast<int>(chunk & 1);
        if (chunk + 1 < n_chunks) load(chunk + 1);
        if (active) {
            const float* ga = gs + b * 16 * pGs + grp * pGs + 16 * wid + col;
            const float* xb = xs + b * 16 * pXs + grp * pXs + col;
            float a4[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) a4[kk] = ga[4 * kk * pGs];
#pragma unroll
            for (int g4 = 0; g4 < kSlSlots / 4; ++g4) {                          // four column tiles at a time: 16 operand reads, then 16 products
                if (4 * g4 < NT) {
                    float bv[4][4];
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                        for (int e = 0; e < 4; ++e) bv[kk][e] = xb[4 * kk * pXs + 16 * (4 * g4 + e)];
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[4 * g4 + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[kk], bv[kk][e], acc[4 * g4 + e], 0, 0, 0);
                }
            }
        }
        if (chunk + 1 < n_chunks) store(b ^ 1);                                 // (the other buffer: its readers passed the barrier below)
        __syncthreads();
    }
    if (!active) return;
    float* slab = partial + (static_cast<int64_t>(blockIdx.x) * 2 + dir) * K4 * N;      // [4H][N]
#pragma unroll
    for (int e = 0; e < kSlSlots; ++e) {
        if (e < NT) {
            const int n = 16 * e + col;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = j0 + 16 * wid + 4 * grp + i;
                if (j < K4 && n < N) slab[static_cast<int64_t>(j) * N + n] = acc[e][i];
            }
        }
    }
}

// d_pos[v][p] = sum over the directions (forward first) and the gate rows j in order of D[dir][j][v] W_ih[dir][j][Dw + p]; row `pad` zero
// (one wave per cell: lane l adds the rows j = l, l + 64, ... of each direction, forward first, then the lanes are added in a fixed tree)
__global__ void __launch_bounds__(64) k_sent_lstm_dpos(const float* __restrict__ cls, const float* __restrict__ w_ih_f,
                                                       const float* __restrict__ w_ih_r, int32_t Dw, int32_t P, int32_t H, int32_t Vp, int32_t pad,
                                                       float* __restrict__ g_pos) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int v = i / P, p = i - v * P, I = Dw + P;
    float sum = 0.f;
    for (int dir = 0; dir < 2; ++dir) {
        const float* w = dir ? w_ih_r : w_ih_f;
        const float* d = cls + static_cast<int64_t>(dir) * 4 * H * Vp;
        float part = 0.f;
        for (int j = lane; j < 4 * H; j += 64) part = fmaf(d[static_cast<int64_t>(j) * Vp + v], w[static_cast<int64_t>(j) * I + Dw + p], part);
        sum += part;
    }
    sum = group_sum<64>(sum);
    if (lane == 0) g_pos[i] = v == pad ? 0.f : sum;
}

struct SlIds { const void* sentence; const void* markers; int64_t ld_sent, ld_mark; const float* table; int32_t Vw; const float* pos; int32_t Vp;
               const int32_t* bits; float scale; };

template <typename IdT, int RT, int UB>
int sl_launch_fwd(const SlIds& x, const float* Wr, int64_t S, int32_t C, int32_t T, int32_t Dw, int32_t P, int32_t H, const SlGeo& g, float* out,
                  float* saved, hipStream_t st) {
    const size_t lds = static_cast<size_t>(2) * 16 * RT * g.pA * 4;
    auto kern = &k_sent_lstm_fwd<IdT, RT, UB>;
    if (!allow_lds(kern, lds)) return RECON_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(ceil_div64(S, 16 * RT)), 2), dim3(kSlThreads), lds, st, static_cast<const IdT*>(x.sentence),
                       x.ld_sent, static_cast<const IdT*>(x.markers), x.ld_mark, x.table, x.Vw, x.pos, x.Vp, x.bits, x.scale, Wr, g.wr_dir, S, C, T,
                       Dw, P, H, g.Kx, g.K16, g.pA, out, saved);
    return RECON_OK;
}

template <int RT, int UB>
int sl_launch_bptt(const float* Whr, const float* g_out, float* saved, int64_t S, int32_t T, int32_t H, const SlGeo& g, hipStream_t st) {
    const size_t lds = static_cast<size_t>(16) * RT * g.pG * 4;
    auto kern = &k_sent_lstm_bptt<RT, UB>;
    if (!allow_lds(kern, lds)) return RECON_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(ceil_div64(S, 16 * RT)), 2), dim3(kSlThreads), lds, st, Whr, g.whr_dir, g_out, saved, S, T, H,
                       g.K16b, g.pG);
    return RECON_OK;
}

template <typename IdT>
int sl_launch_wgrad(const SlIds& x, const float* saved, int64_t S, int32_t C, int32_t T, int32_t Dw, int32_t P, int32_t H, int64_t per, int32_t G,
                    const SlGeo& g, float* partial, hipStream_t st) {
    const size_t lds = static_cast<size_t>(2) * 16 * (g.pGs + g.pXs) * 4;
    auto kern = &k_sent_lstm_wgrad<IdT>;
    if (!allow_lds(kern, lds)) return RECON_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(G), static_cast<unsigned>(g.JB), 2), dim3(kSlThreads), lds, st,
                       static_cast<const IdT*>(x.sentence), x.ld_sent, static_cast<const IdT*>(x.markers), x.ld_mark, x.table, x.Vw, x.pos, x.Vp, x.bits,
                       x.scale, saved, S, C, T, Dw, P, H, per, g.NT, g.pGs, g.pXs, partial);
    return RECON_OK;
}

// workspace of the backward: Whr | the G slabs | the class sums, each part 256-byte aligned
struct SlBwdWs { size_t whr, partial, cls, total; int64_t per; int32_t G; };
inline SlBwdWs sl_bwd_ws(int64_t S, int32_t H, const SlGeo& g, int32_t Vp) {
    SlBwdWs w;
    split_rows(S, kSlMaxGroups, 1, &w.per, &w.G);
    w.whr = 0;
    w.partial = align_up(static_cast<size_t>(2) * g.whr_dir * 4, 256);
    w.cls = w.partial + align_up(static_cast<size_t>(w.G) * 2 * 4 * H * g.N * 4, 256);
    w.total = w.cls + align_up(static_cast<size_t>(2) * 4 * H * Vp * 4, 256);
    return w;
}

}  // namespace
}  // namespace recon

extern "C" int recon_sent_lstm_supported(int64_t B, int32_t C, int32_t T, int32_t Dw, int32_t P, int32_t H) {
    if (B < 1 || C < 1 || T < 1 || Dw < 1 || P < 1 || H < 1) return 0;
    if (H > recon::kSlMaxH || Dw > recon::kSlMaxI || P > recon::kSlMaxI || Dw + P > recon::kSlMaxI || T > (1 << 20)) return 0;
    if (B > (static_cast<int64_t>(1) << 40) / C) return 0;
    const int64_t S = B * C;
    if (S > (static_cast<int64_t>(1) << 40) / (static_cast<int64_t>(T) * 5 * H)) return 0;
    if (ceil_div64(S, 16) > 0x7fffffff) return 0;
    return 1;
}

extern "C" size_t recon_sent_lstm_workspace_bytes(int64_t B, int32_t C, int32_t T, int32_t Dw, int32_t P, int32_t H, int32_t Vp, int32_t backward) {
    if (Vp < 1 || Vp > recon::kSlMaxVp || !recon_sent_lstm_supported(B, C, T, Dw, P, H)) return 0;
    const recon::SlGeo g = recon::sl_geo(Dw, P, H, Vp);
    if (!backward) return align_up(static_cast<size_t>(2) * g.wr_dir * 4, 256);
    return recon::sl_bwd_ws(B * C, H, g, Vp).total;
}

extern "C" size_t recon_sent_lstm_saved_bytes(int64_t B, int32_t C, int32_t T, int32_t Dw, int32_t P, int32_t H) {
    if (!recon_sent_lstm_supported(B, C, T, Dw, P, H)) return 0;
    return recon::lstm_saved_bytes(B * C, T, H);
}

extern "C" int recon_sent_lstm_fwd(const void* sentence, const void* markers, int32_t index_bytes, int64_t ld_sentence, int64_t ld_markers,
                                   const float* word_table, int32_t Vw, const float* pos_table, int32_t Vp, const int32_t* keep_bits,
                                   float keep_scale, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                                   const float* w_ih_rev, const float* w_hh_rev, const float* b_ih_rev, const float* b_hh_rev, int64_t B, int32_t C,
                                   int32_t T, int32_t Dw, int32_t P, int32_t H, float* out, void* saved, void* workspace, size_t workspace_bytes,
                                   recon_stream_t stream) {
    if (B < 0 || C < 0 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (B == 0 || C == 0) return RECON_OK;
    if (!recon_sent_lstm_supported(B, C, T, Dw, P, H) || Vp > recon::kSlMaxVp) return RECON_ERR_UNSUPPORTED;
    if (!sentence || !markers || !word_table || !pos_table || !w_ih || !w_hh || !b_ih || !b_hh || !w_ih_rev || !w_hh_rev || !b_ih_rev || !b_hh_rev ||
        !out || !workspace || Vw < 1 || Vp < 1 || ld_sentence < T || ld_markers < T)
        return RECON_ERR_INVALID;
    if (const int rc = recon::lstm_buffer_checks(workspace, saved, workspace_bytes, recon_sent_lstm_workspace_bytes(B, C, T, Dw, P, H, Vp, 0))) return rc;
    hipStream_t st = as_stream(stream);
    const recon::SlGeo g = recon::sl_geo(Dw, P, H, Vp);
    const int64_t S = B * C;
    float* Wr = static_cast<float*>(workspace);
    hipLaunchKernelGGL(recon::k_sent_lstm_prep_fwd, dim3(static_cast<unsigned>(ceil_div64(2 * g.wr_dir, 256))), dim3(256), 0, st, w_ih, w_hh, b_ih, b_hh,
                       w_ih_rev, w_hh_rev, b_ih_rev, b_hh_rev, g.I, H, g.Kx, g.K16, g.wr_dir, Wr);
    RECON_CHECK_LAUNCH();
    const recon::SlIds x{sentence, markers, ld_sentence, ld_markers, word_table, Vw, pos_table, Vp, keep_bits, keep_scale};
    const int rc = recon::dispatch_ids(index_bytes, [&](auto id) {
        return recon::dispatch_tile(recon::sl_row_tiles(S) == 2, g.UB == 2, [&](auto rt, auto ub) {
            return recon::sl_launch_fwd<typename decltype(id)::type, decltype(rt)::value, decltype(ub)::value>(x, Wr, S, C, T, Dw, P, H, g, out,
                                                                                                              static_cast<float*>(saved), st);
        });
    });
    if (rc != RECON_OK) return rc;
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_sent_lstm_bwd(const void* sentence, const void* markers, int32_t index_bytes, int64_t ld_sentence, int64_t ld_markers,
                                   const float* word_table, int32_t Vw, const float* pos_table, int32_t Vp, const int32_t* keep_bits,
                                   float keep_scale, const float* w_ih, const float* w_hh, const float* w_ih_rev, const float* w_hh_rev,
                                   const float* g_out, void* saved, int64_t B, int32_t C, int32_t T, int32_t Dw, int32_t P, int32_t H,
                                   int32_t pos_padding_idx, float* g_pos_table, float* g_w_ih, float* g_w_hh, float* g_b_ih, float* g_b_hh,
                                   float* g_w_ih_rev, float* g_w_hh_rev, float* g_b_ih_rev, float* g_b_hh_rev, void* workspace,
                                   size_t workspace_bytes, recon_stream_t stream) {
    if (B < 0 || C < 0 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (!recon_sent_lstm_supported(B > 0 ? B : 1, C > 0 ? C : 1, T, Dw, P, H) || Vp > recon::kSlMaxVp) return RECON_ERR_UNSUPPORTED;
    if (!g_pos_table || !g_w_ih || !g_w_hh || !g_b_ih || !g_b_hh || !g_w_ih_rev || !g_w_hh_rev || !g_b_ih_rev || !g_b_hh_rev || Vp < 1)
        return RECON_ERR_INVALID;
    hipStream_t st = as_stream(stream);
    const int32_t I = Dw + P;
    if (B == 0 || C == 0) {
        if (const int rc = recon::zero_fill({{g_pos_table, static_cast<size_t>(Vp) * P}}, st)) return rc;
        return recon::lstm_zero_param_grads(g_w_ih, g_w_hh, g_b_ih, g_b_hh, g_w_ih_rev, g_w_hh_rev, g_b_ih_rev, g_b_hh_rev, I, H, st);
    }
    if (!sentence || !markers || !word_table || !pos_table || !w_ih || !w_hh || !w_ih_rev || !w_hh_rev || !g_out || !saved || !workspace || Vw < 1 ||
        ld_sentence < T || ld_markers < T)
        return RECON_ERR_INVALID;
    if (const int rc = recon::lstm_buffer_checks(workspace, saved, workspace_bytes, recon_sent_lstm_workspace_bytes(B, C, T, Dw, P, H, Vp, 1))) return rc;
    const recon::SlGeo g = recon::sl_geo(Dw, P, H, Vp);
    const int64_t S = B * C;
    const recon::SlBwdWs w = recon::sl_bwd_ws(S, H, g, Vp);
    char* base = static_cast<char*>(workspace);
    float* Whr = reinterpret_cast<float*>(base + w.whr);
    float* partial = reinterpret_cast<float*>(base + w.partial);
    float* cls = reinterpret_cast<float*>(base + w.cls);
    hipLaunchKernelGGL(recon::k_sent_lstm_prep_bwd, dim3(static_cast<unsigned>(ceil_div64(2 * g.whr_dir, 256))), dim3(256), 0, st, w_hh, w_hh_rev, H,
                       g.K16b, g.whr_dir, Whr);
    RECON_CHECK_LAUNCH();
    const int rc_bptt = recon::dispatch_tile(recon::sl_row_tiles(S) == 2, g.UB == 2, [&](auto rt, auto ub) {
        return recon::sl_launch_bptt<decltype(rt)::value, decltype(ub)::value>(Whr, g_out, static_cast<float*>(saved), S, T, H, g, st);
    });
    if (rc_bptt != RECON_OK) return rc_bptt;
    RECON_CHECK_LAUNCH();
    const recon::SlIds x{sentence, markers, ld_sentence, ld_markers, word_table, Vw, pos_table, Vp, keep_bits, keep_scale};
    const int rc = recon::dispatch_ids(index_bytes, [&](auto id) {
        return recon::sl_launch_wgrad<typename decltype(id)::type>(x, static_cast<const float*>(saved), S, C, T, Dw, P, H, w.per, w.G, g, partial, st);
    });
    if (rc != RECON_OK) return rc;
    RECON_CHECK_LAUNCH();
    hipLaunchKernelGGL(recon::k_lstm_reduce, dim3(static_cast<unsigned>(ceil_div64(static_cast<int64_t>(2) * 4 * H * g.N, 256))), dim3(256), 0, st,
                       partial, w.G, I, H, Vp, g_w_ih, g_w_hh, g_b_ih, g_b_hh, g_w_ih_rev, g_w_hh_rev, g_b_ih_rev, g_b_hh_rev, cls);
    RECON_CHECK_LAUNCH();
    hipLaunchKernelGGL(recon::k_sent_lstm_dpos, dim3(static_cast<unsigned>(Vp * P)), dim3(64), 0, st, cls, w_ih,
                       w_ih_rev, Dw, P, H, Vp, pos_padding_idx, g_pos_table);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}
