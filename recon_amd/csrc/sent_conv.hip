// E17 — the sentence convolution and pool of the per-pair baselines CNN and PCNN (models/baselines.py:237-247 and :297-308): three embedding
// gathers, the dropout product, cat, transpose, one to four Conv1d's over the sentence, the max over the positions, the pooled dropout and
// the activation, without x [B][T][Cin], its transpose, any [B][E][T_out] convolution output or a masked copy of one:
//     x[b][t]          = (keep . word[sentence[b][t]] | pt0[positions[b][0][t]] | pt1[positions[b][1][t]])           Cin = Dw + 2 Dp
//     conv_i[b][e][t]  = bias_i[e] + sum_j sum_c w_i[e][c][j] x[b][t + j - pad_i][c]                                 x = 0 outside 0..T-1
//     CNN form:   pad_i = 0, T_out = T - k_i + 1,  pooled[b][i E + e] = max_t conv_i[b][e][t]
//     PCNN form:  one weight, k odd, pad = k / 2, T_out = T,  pooled[b][s E + e] = max_t conv[b][e][t] seg[b][s][t]   (0 where seg is 0)
//     out = act(pool_keep . pooled)
// with the lowest position on an exact tie.  The winning position is kept as one byte per output (255: the maximum was the 0 of a
// zero-factor position), which with out is all the backward needs.
//
// k_sc_pack (once per call): the weights K-major, w_i[e][c][j] -> Wk_i[q][j][cc][Ep] (channel chunk q, pitch CCp, Ep = E rounded up to 16,
//   zeros in the padding), so that a wave's B fragments are rows of 16 consecutive floats.
// k_sc_fwd: workgroup (R rows, 64 output channels, weight i).  x of the R rows is staged in LDS one channel chunk at a time, the rows one
//   behind the other with their zero halo at the pitch CCp = the chunk's K extent per tap: position m's operand row A[m][j CCp + cc] is
//   then LDS[m CCp + (j CCp + cc)] — the convolution is a product of overlapping rows, [R Tp, k CCp] x [k CCp, 64], on
//   v_mfma_f32_16x16x4_f32 with CCp an odd multiple of 4 (a fragment's 16 rows fall on different banks).  Positions that straddle two rows
//   are computed and ignored.  Wave w owns 16 channels and all position tiles (up to 9).  The epilogue goes through LDS: thread (row,
//   segment, channel) walks the positions upwards: bias, segment factor, the first maximum, pool_keep, the activation, the store, the byte.
// k_sc_bwd_w: workgroup (row group z, 32 output channels, weight i) walks its rows upwards; a row's x (one channel chunk of it) and its
//   32 (x 3 segments) values of g f and positions are staged in LDS; a thread owns two (c, j) cells x 32 channels of the slab
//   (d_w | d_bias) in registers.  k_sc_bwd_pos: workgroup (row group), weight by weight (its position columns staged in LDS where they
//   fit), forms the position columns of d_x of a row, [T][2 Dp], and folds them into its LDS slab [2][P][Dp]: a thread per slab cell walks
//   the row's positions upwards.  k_sc_reduce adds the slabs in group order.  fp32 throughout, no atomics.
#include "recon_common.h"

#include <cmath>

namespace recon {
namespace {

constexpr int kScNT = 256;
constexpr int kScMaxT = 128, kScMaxCin = 320, kScMaxE = 1024, kScMaxK = 9, kScMaxW = 4;   // MAX_T, MAX_CIN, MAX_E, MAX_K, MAX_WEIGHTS of recon_amd/sentence_conv.py
constexpr int kScChunk = 100;                    // channels of a staged chunk of the forward (its pitch: 100 = 4 x 25)
constexpr int kScMaxMT = 9;                      // 16-position tiles of a workgroup
constexpr int kScLdsFloats = 15360;              // 60 KiB of dynamic LDS
constexpr int kScETile = 64;
constexpr int kScCsLd = kScETile + 1;
constexpr int kScNone = 255;
constexpr int kScMaxGroups = 32;                 // row groups of the weight-gradient slabs
constexpr int64_t kScSlabFloats = int64_t{1} << 24;      // cap of all slabs together (64 MiB): fewer groups above it
constexpr int kScPosGroups = 256;                // row groups of the position-table slabs
constexpr int kScBwdE = 32, kScBwdCells = 512, kScBwdXFloats = 8192;
constexpr int kScPosSlabFloats = 4096, kScPosDxFloats = 4096;
using sc_f32x4 = __attribute__((ext_vector_type(4))) float;

struct ScIn {
    const void* sent; const void* posi; const float* word; const float* pt0; const float* pt1;
    const uint32_t* keep_bits; const float* keep_f; const float* seg; const float* pool_keep;
    float keep_scale;
    int32_t sent_es, pos_es, V, P, T, Dw, Dp, Cin, E, n, segmented, act, KW;
    int32_t k[kScMaxW];
    int64_t B;
};

struct ScGeo { int32_t nq, CC, CCp, Ep, R, MT, rows, lds_floats; int64_t woff[kScMaxW + 1]; };

inline int sc_pitch(int c) { int p = (c + 3) / 4; if (!(p & 1)) ++p; return 4 * p; }
inline int sc_pad(const ScIn& a, int i) { return a.segmented ? a.k[i] / 2 : 0; }

ScGeo sc_geo(const ScIn& a) {
    ScGeo g;
    if (a.Cin <= kScChunk) { g.nq = 1; g.CC = a.Cin; g.CCp = sc_pitch(a.Cin); }
    else { g.CC = kScChunk; g.CCp = kScChunk; g.nq = (a.Cin + kScChunk - 1) / kScChunk; }
    g.Ep = (a.E + 15) / 16 * 16;
    int kmax = 1;
    g.woff[0] = 0;
    for (int i = 0; i < a.n; ++i) {
        kmax = a.k[i] > kmax ? a.k[i] : kmax;
        g.woff[i + 1] = g.woff[i] + static_cast<int64_t>(g.nq) * a.k[i] * g.CCp * g.Ep;
    }
    const int Tp = a.T + 2 * sc_pad(a, 0);
    int R = 1;
    while (true) {                                                        // the most rows whose tiles and staged chunk fit
        const int mt = ((R + 1) * Tp + 15) / 16;
        if (mt > kScMaxMT || (mt * 16 + kmax - 1) * g.CCp > kScLdsFloats) break;
        ++R;
    }
    g.R = R;
    g.MT = (R * Tp + 15) / 16;
    g.rows = g.MT * 16 + kmax - 1;
    const int cs = g.MT * 16 * kScCsLd;
    g.lds_floats = g.rows * g.CCp > cs ? g.rows * g.CCp : cs;
    return g;
}

__device__ __forceinline__ int64_t sc_id(const void* p, int es, int64_t i) {
    return es == 8 ? static_cast<const int64_t*>(p)[i] : (es == 4 ? static_cast<const int32_t*>(p)[i] : static_cast<const int8_t*>(p)[i]);
}
// x[b][t][c]; an id outside its table reads row 0 and raises `bad`
__device__ __forceinline__ float sc_x(const ScIn& a, int64_t b, int t, int c, bool& bad) {
    if (c < a.Dw) {
        int64_t id = sc_id(a.sent, a.sent_es, b * a.T + t);
        if (id < 0 || id >= a.V) { bad = true; id = 0; }
        float v = a.word[id * a.Dw + c];
        if (a.keep_bits) v = ((a.keep_bits[(b * a.T + t) * a.KW + (c >> 5)] >> (c & 31)) & 1u) ? v * a.keep_scale : 0.f;
        else if (a.keep_f) v *= a.keep_f[(b * a.T + t) * a.Dw + c];
        return v;
    }
    const int cp = c - a.Dw, tbl = cp >= a.Dp ? 1 : 0;
    int64_t id = sc_id(a.posi, a.pos_es, (b * 2 + tbl) * a.T + t);
    if (id < 0 || id >= a.P) { bad = true; id = 0; }
    return (tbl ? a.pt1 : a.pt0)[id * a.Dp + cp - tbl * a.Dp];
}

struct ScPack { const float* w[kScMaxW]; float* packed; int64_t woff[kScMaxW + 1]; int32_t nq, CC, CCp, Ep; };

__global__ void __launch_bounds__(kScNT) k_sc_pack(const ScIn a, const ScPack p) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * kScNT + threadIdx.x;
    if (idx >= p.woff[a.n]) return;
    int i = 0;
    while (idx >= p.woff[i + 1]) ++i;
    int64_t r = idx - p.woff[i];
    const int k = a.k[i];
    const int e = static_cast<int>(r % p.Ep);
    r /= p.Ep;
    const int cc = static_cast<int>(r % p.CCp);
    r /= p.CCp;
    const int j = static_cast<int>(r % k), q = static_cast<int>(r / k);
    const int c = q * p.CC + cc;
    p.packed[idx] = (cc < p.CC && c < a.Cin && e < a.E) ? p.w[i][(static_cast<int64_t>(e) * a.Cin + c) * k + j] : 0.f;
}

struct ScFwd { const float* packed; const float* bias[kScMaxW]; float* out; uint8_t* at; int32_t* status; ScGeo g; };

// grid: (ceil(B / R), ceil(E / 64), weights)
__global__ void __launch_bounds__(kScNT) k_sc_fwd(const ScIn a, const ScFwd f) {
    extern __shared__ __align__(16) float sc_lds[];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 15, g = lane >> 4;
    const int wi = blockIdx.z, k = a.k[wi], pad = a.segmented ? k / 2 : 0, Tp = a.T + 2 * pad, Tout = a.segmented ? a.T : a.T - k + 1;
    const int64_t b0 = static_cast<int64_t>(blockIdx.x) * f.g.R;
    const int Rn = static_cast<int>(min(static_cast<int64_t>(f.g.R), a.B - b0));
    const int MT = (Rn * Tp + 15) >> 4, rows = MT * 16 + k - 1;
    const int CCp = f.g.CCp, CC = f.g.CC, Ep = f.g.Ep;
    const int e0 = blockIdx.y * kScETile + w * 16;
    const bool active = e0 < Ep;
    bool bad = false;
    sc_f32x4 acc[kScMaxMT];
#pragma unroll
    for (int mt = 0; mt < kScMaxMT; ++mt) acc[mt] = sc_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < f.g.nq; ++q) {
        if (q) __syncthreads();
        for (int idx = t; idx < rows * CCp; idx += kScNT) {
            const int m = idx / CCp, cc = idx - m * CCp, r = m / Tp, tt = m - r * Tp - pad, c = q * CC + cc;
            float v = 0.f;
            if (r < Rn && tt >= 0 && tt < a.T && cc < CC && c < a.Cin) v = sc_x(a, b0 + r, tt, c, bad);
            sc_lds[idx] = v;
        }
        __syncthreads();
        if (active) {
            const float* __restrict__ wk = f.packed + f.g.woff[wi] + static_cast<int64_t>(q) * k * CCp * Ep + e0 + li;
            const float* __restrict__ xa = sc_lds + li * CCp + g;
            const int K = k * CCp;
            float bv = wk[static_cast<int64_t>(g) * Ep];
            // One tap (CCp terms) at a time into `part`, then added to the total: a chain of k Cin fma's (909 at k = 9, Cin = 101) in one
            // accumulator drifts past 2^-20 of the largest output; chains of at most 100 and k nq adds do not.
            for (int k0 = 0; k0 < K; k0 += CCp) {
                sc_f32x4 part[kScMaxMT];
#pragma unroll
                for (int mt = 0; mt < kScMaxMT; ++mt) part[mt] = sc_f32x4{0.f, 0.f, 0.f, 0.f};
                for (int kk = k0; kk < k0 + CCp; kk += 4) {              // (the next step's fragment of the weights is asked for first)
                    const float nb = wk[static_cast<int64_t>(kk + 4 < K ? kk + 4 + g : g) * Ep];
#pragma unroll
                    for (int mt = 0; mt < kScMaxMT; ++mt)
                        if (mt < MT) part[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[mt * 16 * CCp + kk], bv, part[mt], 0, 0, 0);
                    bv = nb;
                }
#pragma unroll
                for (int mt = 0; mt < kScMaxMT; ++mt)
                    if (mt < MT) acc[mt] += part[mt];
            }
        }
    }
    __syncthreads();
    // C layout: column = lane & 15, row = 4 (lane >> 4) + r
    if (active)
#pragma unroll
        for (int mt = 0; mt < kScMaxMT; ++mt)
            if (mt < MT)
#pragma unroll
                for (int r = 0; r < 4; ++r) sc_lds[(mt * 16 + 4 * g + r) * kScCsLd + w * 16 + li] = acc[mt][r];
    __syncthreads();
    const int nslot = a.segmented ? 3 : 1, nE = (a.segmented ? 3 : a.n) * a.E;
    for (int task = t; task < Rn * nslot * kScETile; task += kScNT) {
        const int el = task & (kScETile - 1), rs = task >> 6, r = rs / nslot, slot = rs - r * nslot;
        const int e = blockIdx.y * kScETile + el;
        if (e >= a.E) continue;
        const int64_t b = b0 + r;
        const float bias = f.bias[wi][e];
        const float* __restrict__ cv = sc_lds + r * Tp * kScCsLd + el;
        const float* __restrict__ sg = a.segmented ? a.seg + (b * 3 + slot) * a.T : nullptr;
        float best = 0.f;
        int at = kScNone;
        for (int tt = 0; tt < Tout; ++tt) {
            float v = cv[tt * kScCsLd] + bias;
            bool zero = false;
            if (sg) {
                const float fct = sg[tt];
                zero = fct == 0.f;
                v = zero ? 0.f : v * fct;
            }
            const bool take = tt == 0 || v > best;
            best = take ? v : best;
            at = take ? (zero ? kScNone : tt) : at;
        }
        const int64_t col = b * nE + (a.segmented ? slot : wi) * a.E + e;
        if (a.pool_keep) best *= a.pool_keep[col];
        if (a.act == 1) best = tanhf(best);
        else if (a.act == 2) best = best > 0.f ? best : 0.f;
        f.out[col] = best;
        if (f.at) f.at[col] = static_cast<uint8_t>(at);
    }
    if (bad) f.status[0] = 1;
}

struct ScBwd {
    const float* w[kScMaxW]; const float* out; const uint8_t* at; const float* g_out;
    float* slabs; float* pos_slabs; int64_t soff[kScMaxW + 1];             // float offsets of d_w_i in a slab; the biases behind soff[n]
    int64_t slab; int64_t per, per_pos; int32_t pad_idx;
};

// g_out act'(out) pool_keep f of output column (slot, e) of row b and its position; (0, 0) where there is no gradient
__device__ __forceinline__ float sc_gf(const ScIn& a, const ScBwd& p, int64_t b, int slot, int e, int& pos) {
    const int nE = (a.segmented ? 3 : a.n) * a.E;
    const int64_t col = b * nE + slot * a.E + e;
    const int at = p.at[col];
    pos = 0;
    if (at == kScNone) return 0.f;
    const int last = (a.segmented ? a.T : a.T - a.k[a.segmented ? 0 : slot] + 1) - 1;
    pos = at < last ? at : last;                                         // (a byte this library did not write is never used as an address)
    const float o = p.out[col];
    float gv = p.g_out[col];
    if (a.act == 1) gv *= 1.f - o * o;
    else if (a.act == 2) gv = o > 0.f ? gv : 0.f;
    if (a.pool_keep) gv *= a.pool_keep[col];
    if (a.segmented) gv *= a.seg[(b * 3 + slot) * a.T + pos];
    return gv;
}

// grid: (row groups, ceil(E / 32), weights)
__global__ void __launch_bounds__(kScNT) k_sc_bwd_w(const ScIn a, const ScBwd p) {
    extern __shared__ __align__(16) float sc_xs[];
    __shared__ float gs[3 * kScBwdE];
    __shared__ int ps[3 * kScBwdE];
    const int t = threadIdx.x;
    const int wi = blockIdx.z, k = a.k[wi], pad = a.segmented ? k / 2 : 0, Tp = a.T + 2 * pad;
    const int e0 = blockIdx.y * kScBwdE, nslot = a.segmented ? 3 : 1;
    const int64_t z = blockIdx.x, b_lo = z * p.per, b_hi = min(a.B, b_lo + p.per);
    int CCb = a.Cin;
    CCb = min(CCb, kScBwdCells / k);
    CCb = min(CCb, kScBwdXFloats / Tp - 1);
    const int pitch = CCb | 1;
    float* __restrict__ mine = p.slabs + z * p.slab;
    bool bad = false;
    for (int c0 = 0; c0 < a.Cin; c0 += CCb) {
        const int ccn = min(CCb, a.Cin - c0);
        int cc[2], jj[2];
        bool ok[2];
        float acc[2][kScBwdE];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int r = t + s * kScNT;
            ok[s] = r < ccn * k;
            cc[s] = ok[s] ? r / k : 0;
            jj[s] = ok[s] ? r - cc[s] * k : 0;
#pragma unroll
            for (int el = 0; el < kScBwdE; ++el) acc[s][el] = 0.f;
        }
        float bacc = 0.f;
        for (int64_t b = b_lo; b < b_hi; ++b) {
            __syncthreads();
            for (int idx = t; idx < Tp * ccn; idx += kScNT) {
                const int row = idx / ccn, c = idx - row * ccn, tt = row - pad;
                sc_xs[row * pitch + c] = (tt >= 0 && tt < a.T) ? sc_x(a, b, tt, c0 + c, bad) : 0.f;
            }
            if (t < nslot * kScBwdE) {
                const int slot = t / kScBwdE, el = t - slot * kScBwdE;
                int pos = 0;
                gs[t] = e0 + el < a.E ? sc_gf(a, p, b, a.segmented ? slot : wi, e0 + el, pos) : 0.f;
                ps[t] = pos;
            }
            __syncthreads();
            for (int slot = 0; slot < nslot; ++slot) {
#pragma unroll
                for (int el = 0; el < kScBwdE; ++el) {
                    const float gv = gs[slot * kScBwdE + el];
                    const float* __restrict__ xr = sc_xs + ps[slot * kScBwdE + el] * pitch;
#pragma unroll
                    for (int s = 0; s < 2; ++s) acc[s][el] = fmaf(gv, xr[jj[s] * pitch + cc[s]], acc[s][el]);
                }
                if (c0 == 0 && t < kScBwdE) bacc += gs[slot * kScBwdE + t];
            }
        }
        const int64_t Rw = static_cast<int64_t>(a.Cin) * k;
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (ok[s])
#pragma unroll
                for (int el = 0; el < kScBwdE; ++el)
                    if (e0 + el < a.E) mine[p.soff[wi] + (e0 + el) * Rw + static_cast<int64_t>(c0 + cc[s]) * k + jj[s]] = acc[s][el];
        if (c0 == 0 && t < kScBwdE && e0 + t < a.E) mine[p.soff[a.n] + wi * a.E + e0 + t] = bacc;
    }
}

// The LDS of k_sc_bwd_pos in floats: slab [2][P][Dp] | dx [T][2 Dp] | g f of one weight's outputs | that weight's position columns
// (where they fit) | the row's position ids | the positions' bytes
struct ScPosLds { int32_t cells, dx, gs, wl, ids, ps, total; bool wlds; };
ScPosLds sc_pos_lds(const ScIn& a) {
    ScPosLds l;
    int kmax = 1;
    for (int i = 0; i < a.n; ++i) kmax = a.k[i] > kmax ? a.k[i] : kmax;
    const int nsl = a.segmented ? 3 : 1;
    l.cells = 2 * a.P * a.Dp;
    l.dx = 2 * a.T * a.Dp;
    l.gs = nsl * a.E;
    l.ids = 2 * a.T;
    l.ps = (nsl * a.E + 3) / 4;
    const int base = l.cells + l.dx + l.gs + l.ids + l.ps;
    const int64_t wl = static_cast<int64_t>(a.E) * 2 * a.Dp * kmax;
    l.wlds = base + wl <= kScLdsFloats;
    l.wl = l.wlds ? static_cast<int32_t>(wl) : 0;
    l.total = base + l.wl;
    return l;
}

// grid: row groups of the position tables.  WLDS: the position columns of the current weight, [E][2 Dp][k], are staged in LDS
template <bool WLDS>
__global__ void __launch_bounds__(kScNT) k_sc_bwd_pos(const ScIn a, const ScBwd p, const ScPosLds l) {
    extern __shared__ __align__(16) float sc_pos[];
    float* slab = sc_pos;
    float* dx = slab + l.cells;
    float* gs = dx + l.dx;
    float* wl = gs + l.gs;
    int* ids = reinterpret_cast<int*>(wl + l.wl);
    uint8_t* ps = reinterpret_cast<uint8_t*>(ids + l.ids);
    const int t = threadIdx.x;
    const int nsl = a.segmented ? 3 : 1, D2 = 2 * a.Dp, half = a.P * a.Dp;
    const int64_t z = blockIdx.x, b_lo = z * p.per_pos, b_hi = min(a.B, b_lo + p.per_pos);
    for (int i = t; i < l.cells; i += kScNT) slab[i] = 0.f;
    for (int wi = 0; wi < a.n; ++wi) {
        const int k = a.k[wi], pad = a.segmented ? k / 2 : 0, W = D2 * k;
        const int64_t Rw = static_cast<int64_t>(a.Cin) * k;
        const float* __restrict__ wg = p.w[wi] + static_cast<int64_t>(a.Dw) * k;      // row e's position columns: W consecutive floats at e Rw
        if constexpr (WLDS) {
            __syncthreads();                                             // the previous weight's columns have been read
            for (int i = t; i < a.E * W; i += kScNT) {
                const int e = i / W;
                wl[i] = wg[e * Rw + (i - e * W)];
            }
        }
        for (int64_t b = b_lo; b < b_hi; ++b) {
            __syncthreads();                                             // the previous row's dx, ids and g f have been read
            for (int i = t; i < nsl * a.E; i += kScNT) {
                const int sl = i / a.E;
                int pos = 0;
                gs[i] = sc_gf(a, p, b, a.segmented ? sl : wi, i - sl * a.E, pos);
                ps[i] = static_cast<uint8_t>(pos);
            }
            for (int i = t; i < 2 * a.T; i += kScNT) {
                int64_t id = sc_id(a.posi, a.pos_es, b * 2 * a.T + i);
                ids[i] = (id < 0 || id >= a.P) ? 0 : static_cast<int>(id);
            }
            __syncthreads();
            for (int idx = t; idx < a.T * D2; idx += kScNT) {
                const int tt = idx / D2, c2 = idx - tt * D2;
                float s = 0.f;
                for (int sl = 0; sl < nsl; ++sl) {
                    const float* gsl = gs + sl * a.E;
                    const uint8_t* psl = ps + sl * a.E;
#pragma unroll 8
                    for (int e = 0; e < a.E; ++e) {                       // selects: the reads of the next channels go ahead
                        const int j = tt - psl[e] + pad;
                        const bool hit = j >= 0 && j < k;
                        const int at = c2 * k + (hit ? j : 0);
                        const float wv = WLDS ? wl[e * W + at] : wg[e * Rw + at];
                        s = hit ? fmaf(gsl[e], wv, s) : s;
                    }
                }
                dx[idx] = s;
            }
            __syncthreads();
            // a thread per slab cell (table, id, column) walks the row's positions upwards: one order, no two writers
            for (int cell = t; cell < l.cells; cell += kScNT) {
                const int tbl = cell >= half ? 1 : 0, rem = cell - tbl * half, id = rem / a.Dp, d = rem - id * a.Dp;
                if (id == p.pad_idx) continue;
                float s = slab[cell];
                const int* row = ids + tbl * a.T;
                const float* col = dx + tbl * a.Dp + d;
                for (int tt = 0; tt < a.T; ++tt) s = row[tt] == id ? s + col[tt * D2] : s;
                slab[cell] = s;
            }
        }
    }
    __syncthreads();
    for (int i = t; i < l.cells; i += kScNT) p.pos_slabs[z * l.cells + i] = slab[i];
}

struct ScRed { float* g_w[kScMaxW]; float* g_b[kScMaxW]; float* g_pt0; float* g_pt1; int32_t G, Gp; };

__global__ void __launch_bounds__(kScNT) k_sc_reduce(const ScIn a, const ScBwd p, const ScRed r) {
    const int64_t q = static_cast<int64_t>(blockIdx.x) * kScNT + threadIdx.x;
    const int cells = 2 * a.P * a.Dp;
    if (q < p.slab) {
        if (!p.slabs) return;
        float s = 0.f;
#pragma unroll 8
        for (int z = 0; z < r.G; ++z) s += p.slabs[z * p.slab + q];
        if (q >= p.soff[a.n]) {
            const int64_t i = (q - p.soff[a.n]) / a.E;
            if (r.g_b[i]) r.g_b[i][q - p.soff[a.n] - i * a.E] = s;
        } else {
            int i = 0;
            while (q >= p.soff[i + 1]) ++i;
            if (r.g_w[i]) r.g_w[i][q - p.soff[i]] = s;
        }
    } else if (q < p.slab + cells) {
        if (!p.pos_slabs) return;
        const int64_t c = q - p.slab;
        float s = 0.f;
#pragma unroll 8
        for (int z = 0; z < r.Gp; ++z) s += p.pos_slabs[static_cast<int64_t>(z) * cells + c];
        const int64_t half = static_cast<int64_t>(a.P) * a.Dp;
        if (c < half) { if (r.g_pt0) r.g_pt0[c] = s; }
        else if (r.g_pt1) r.g_pt1[c - half] = s;
    }
}

// 0 ok, RECON_ERR_INVALID or RECON_ERR_UNSUPPORTED for the shape alone
int sc_shape(int64_t B, int32_t T, int32_t Dw, int32_t Dp, int32_t P, int32_t E, const int32_t* ks, int32_t n, int32_t segmented) {
    if (B < 0 || T < 1 || Dw < 1 || Dp < 1 || P < 1 || E < 1 || n < 1 || !ks) return RECON_ERR_INVALID;
    if (n > kScMaxW) return RECON_ERR_UNSUPPORTED;
    for (int i = 0; i < n; ++i)
        if (ks[i] < 1 || (!segmented && ks[i] > T)) return RECON_ERR_INVALID;
    if (segmented && (n != 1 || !(ks[0] & 1))) return RECON_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (ks[i] > kScMaxK) return RECON_ERR_UNSUPPORTED;
    if (B > (int64_t{1} << 24) || T > kScMaxT || Dw + 2 * static_cast<int64_t>(Dp) > kScMaxCin || E > kScMaxE) return RECON_ERR_UNSUPPORTED;
    if (2 * static_cast<int64_t>(P) * Dp > kScPosSlabFloats || 2 * static_cast<int64_t>(T) * Dp > kScPosDxFloats) return RECON_ERR_UNSUPPORTED;
    return RECON_OK;
}

ScIn sc_in(int64_t B, int32_t T, int32_t Dw, int32_t Dp, int32_t P, int32_t E, const int32_t* ks, int32_t n, int32_t segmented) {
    ScIn a{};
    a.B = B; a.T = T; a.Dw = Dw; a.Dp = Dp; a.P = P; a.E = E; a.n = n; a.segmented = segmented; a.Cin = Dw + 2 * Dp; a.KW = (Dw + 31) / 32;
    for (int i = 0; i < n; ++i) a.k[i] = ks[i];
    return a;
}

struct ScBwdGeo { int64_t soff[kScMaxW + 1]; int64_t slab, per, G, per_pos, Gp, cells; };
ScBwdGeo sc_bwd_geo(const ScIn& a) {
    ScBwdGeo g;
    g.soff[0] = 0;
    for (int i = 0; i < a.n; ++i) g.soff[i + 1] = g.soff[i] + static_cast<int64_t>(a.E) * a.Cin * a.k[i];
    g.slab = g.soff[a.n] + static_cast<int64_t>(a.n) * a.E;
    int64_t G = kScSlabFloats / g.slab;
    G = G < 1 ? 1 : (G > kScMaxGroups ? kScMaxGroups : G);
    G = a.B < G ? a.B : G;
    g.per = G ? ceil_div64(a.B, G) : 1;
    g.G = G ? ceil_div64(a.B, g.per) : 0;
    int64_t Gp = a.B < kScPosGroups ? a.B : kScPosGroups;
    g.per_pos = Gp ? ceil_div64(a.B, Gp) : 1;
    g.Gp = Gp ? ceil_div64(a.B, g.per_pos) : 0;
    g.cells = 2 * static_cast<int64_t>(a.P) * a.Dp;
    return g;
}

bool sc_aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace
}  // namespace recon

extern "C" int recon_sent_conv_supported(int64_t B, int32_t T, int32_t Dw, int32_t Dp, int32_t P, int32_t E, const int32_t* ks, int32_t n,
                                         int32_t segmented) {
    return recon::sc_shape(B, T, Dw, Dp, P, E, ks, n, segmented) == RECON_OK ? 1 : 0;
}

extern "C" size_t recon_sent_conv_workspace_bytes(int64_t B, int32_t T, int32_t Dw, int32_t Dp, int32_t P, int32_t E, const int32_t* ks, int32_t n,
                                                  int32_t segmented, int32_t backward) {
    using namespace recon;
    if (sc_shape(B, T, Dw, Dp, P, E, ks, n, segmented) != RECON_OK || B == 0) return 0;
    const ScIn a = sc_in(B, T, Dw, Dp, P, E, ks, n, segmented);
    if (!backward) return align_up(static_cast<size_t>(sc_geo(a).woff[n]) * sizeof(float), 16);
    const ScBwdGeo g = sc_bwd_geo(a);
    return align_up(static_cast<size_t>(g.G * g.slab + g.Gp * g.cells) * sizeof(float), 16);
}

namespace recon {
namespace {
// the checks and the argument block the two entries share
int sc_args(ScIn& a, const void* sentence, int32_t sentence_bytes, const void* positions, int32_t position_bytes, const float* word_table, int32_t V,
            const float* pos_table_0, const float* pos_table_1, const void* keep_bits, float keep_scale, const float* keep_factors,
            const float* segments, const void* const* weights, const void* const* biases, const int32_t* ks, int32_t n, const float* pool_keep,
            int32_t activation, int64_t B, int32_t T, int32_t Dw, int32_t Dp, int32_t P, int32_t E) {
    const int rc = sc_shape(B, T, Dw, Dp, P, E, ks, n, segments != nullptr);
    if (rc != RECON_OK) return rc;
    if (V < 1 || activation < 0 || activation > 2 || (sentence_bytes != 4 && sentence_bytes != 8) ||
        (position_bytes != 1 && position_bytes != 4 && position_bytes != 8) || (keep_bits && keep_factors))
        return RECON_ERR_INVALID;
    a = sc_in(B, T, Dw, Dp, P, E, ks, n, segments != nullptr);
    if (B == 0) return RECON_OK;
    if (!sentence || !positions || !word_table || !pos_table_0 || !pos_table_1 || !weights || !biases) return RECON_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (!weights[i] || !biases[i]) return RECON_ERR_INVALID;
    a.sent = sentence; a.sent_es = sentence_bytes; a.posi = positions; a.pos_es = position_bytes; a.word = word_table; a.V = V;
    a.pt0 = pos_table_0; a.pt1 = pos_table_1; a.keep_bits = static_cast<const uint32_t*>(keep_bits); a.keep_scale = keep_scale;
    a.keep_f = keep_factors; a.seg = segments; a.pool_keep = pool_keep; a.act = activation;
    return RECON_OK;
}
}  // namespace
}  // namespace recon

extern "C" int recon_sent_conv_fwd(const void* sentence, int32_t sentence_bytes, const void* positions, int32_t position_bytes,
                                   const float* word_table, int32_t V, const float* pos_table_0, const float* pos_table_1, int32_t P,
                                   const void* keep_bits, float keep_scale, const float* keep_factors, const float* segments,
                                   const void* const* weights, const void* const* biases, const int32_t* ks, int32_t n, const float* pool_keep,
                                   int32_t activation, int64_t B, int32_t T, int32_t Dw, int32_t Dp, int32_t E, float* out, void* max_at,
                                   int32_t* status, void* workspace, size_t workspace_bytes, recon_stream_t stream) {
    using namespace recon;
    ScIn a;
    const int rc = sc_args(a, sentence, sentence_bytes, positions, position_bytes, word_table, V, pos_table_0, pos_table_1, keep_bits, keep_scale,
                           keep_factors, segments, weights, biases, ks, n, pool_keep, activation, B, T, Dw, Dp, P, E);
    if (rc != RECON_OK || B == 0) return rc;
    if (!out || !status || !workspace || !sc_aligned16(workspace)) return RECON_ERR_INVALID;
    if (workspace_bytes < recon_sent_conv_workspace_bytes(B, T, Dw, Dp, P, E, ks, n, a.segmented, 0)) return RECON_ERR_WORKSPACE;
    const ScGeo g = sc_geo(a);
    hipStream_t st = as_stream(stream);
    ScPack pk{};
    ScFwd f{};
    for (int i = 0; i < n; ++i) {
        pk.w[i] = static_cast<const float*>(weights[i]);
        f.bias[i] = static_cast<const float*>(biases[i]);
    }
    for (int i = 0; i <= n; ++i) pk.woff[i] = g.woff[i];
    pk.packed = static_cast<float*>(workspace);
    pk.nq = g.nq; pk.CC = g.CC; pk.CCp = g.CCp; pk.Ep = g.Ep;
    hipLaunchKernelGGL(k_sc_pack, dim3(static_cast<unsigned>(ceil_div64(g.woff[n], kScNT))), dim3(kScNT), 0, st, a, pk);
    RECON_CHECK_LAUNCH();
    f.packed = pk.packed; f.out = out; f.at = static_cast<uint8_t*>(max_at); f.status = status; f.g = g;
    const dim3 grid(static_cast<unsigned>(ceil_div64(B, g.R)), static_cast<unsigned>((E + kScETile - 1) / kScETile), static_cast<unsigned>(n));
    hipLaunchKernelGGL(k_sc_fwd, grid, dim3(kScNT), sizeof(float) * g.lds_floats, st, a, f);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_sent_conv_bwd(const void* sentence, int32_t sentence_bytes, const void* positions, int32_t position_bytes,
                                   const float* word_table, int32_t V, const float* pos_table_0, const float* pos_table_1, int32_t P,
                                   const void* keep_bits, float keep_scale, const float* keep_factors, const float* segments,
                                   const void* const* weights, const int32_t* ks, int32_t n, const float* pool_keep, int32_t activation, int64_t B,
                                   int32_t T, int32_t Dw, int32_t Dp, int32_t E, const float* out, const void* max_at, const float* g_out,
                                   int32_t pos_padding_idx, float* g_pos_table_0, float* g_pos_table_1, void* const* g_weights,
                                   void* const* g_biases, void* workspace, size_t workspace_bytes, recon_stream_t stream) {
    using namespace recon;
    ScIn a;
    const int rc = sc_args(a, sentence, sentence_bytes, positions, position_bytes, word_table, V, pos_table_0, pos_table_1, keep_bits, keep_scale,
                           keep_factors, segments, weights, weights, ks, n, pool_keep, activation, B, T, Dw, Dp, P, E);
    if (rc != RECON_OK) return rc;
    hipStream_t st = as_stream(stream);
    bool params = false;
    for (int i = 0; i < n; ++i) params = params || (g_weights && g_weights[i]) || (g_biases && g_biases[i]);
    const bool tables = g_pos_table_0 || g_pos_table_1;
    if (B == 0) {                                                        // zeros in every wanted gradient, no kernel
        const size_t tb = sizeof(float) * P * Dp;
        if (g_pos_table_0 && hipMemsetAsync(g_pos_table_0, 0, tb, st) != hipSuccess) return RECON_ERR_LAUNCH;
        if (g_pos_table_1 && hipMemsetAsync(g_pos_table_1, 0, tb, st) != hipSuccess) return RECON_ERR_LAUNCH;
        for (int i = 0; i < n; ++i) {
            if (g_weights && g_weights[i] && hipMemsetAsync(g_weights[i], 0, sizeof(float) * E * a.Cin * ks[i], st) != hipSuccess) return RECON_ERR_LAUNCH;
            if (g_biases && g_biases[i] && hipMemsetAsync(g_biases[i], 0, sizeof(float) * E, st) != hipSuccess) return RECON_ERR_LAUNCH;
        }
        return RECON_OK;
    }
    if (!params && !tables) return RECON_OK;
    if (!out || !max_at || !g_out) return RECON_ERR_INVALID;
    if (!workspace || !sc_aligned16(workspace)) return RECON_ERR_INVALID;
    if (workspace_bytes < recon_sent_conv_workspace_bytes(B, T, Dw, Dp, P, E, ks, n, a.segmented, 1)) return RECON_ERR_WORKSPACE;
    const ScBwdGeo g = sc_bwd_geo(a);
    ScBwd p{};
    ScRed r{};
    for (int i = 0; i < n; ++i) {
        p.w[i] = static_cast<const float*>(weights[i]);
        r.g_w[i] = g_weights ? static_cast<float*>(g_weights[i]) : nullptr;
        r.g_b[i] = g_biases ? static_cast<float*>(g_biases[i]) : nullptr;
    }
    for (int i = 0; i <= n; ++i) p.soff[i] = g.soff[i];
    p.out = out; p.at = static_cast<const uint8_t*>(max_at); p.g_out = g_out; p.slab = g.slab; p.per = g.per; p.per_pos = g.per_pos;
    p.pad_idx = pos_padding_idx;
    p.slabs = params ? static_cast<float*>(workspace) : nullptr;
    p.pos_slabs = tables ? static_cast<float*>(workspace) + g.G * g.slab : nullptr;
    r.g_pt0 = g_pos_table_0; r.g_pt1 = g_pos_table_1; r.G = static_cast<int32_t>(g.G); r.Gp = static_cast<int32_t>(g.Gp);
    if (params) {
        int kmax = 1;
        for (int i = 0; i < n; ++i) kmax = ks[i] > kmax ? ks[i] : kmax;
        // (the largest staged chunk of any weight: rows Tp, pitch CCb | 1)
        size_t lds = 0;
        for (int i = 0; i < n; ++i) {
            const int Tp = T + 2 * sc_pad(a, i);
            int CCb = a.Cin;
            CCb = CCb < kScBwdCells / ks[i] ? CCb : kScBwdCells / ks[i];
            CCb = CCb < kScBwdXFloats / Tp - 1 ? CCb : kScBwdXFloats / Tp - 1;
            const size_t need = sizeof(float) * Tp * (CCb | 1);
            lds = need > lds ? need : lds;
        }
        const dim3 grid(static_cast<unsigned>(g.G), static_cast<unsigned>((E + kScBwdE - 1) / kScBwdE), static_cast<unsigned>(n));
        hipLaunchKernelGGL(k_sc_bwd_w, grid, dim3(kScNT), lds, st, a, p);
        RECON_CHECK_LAUNCH();
    }
    if (tables) {
        const ScPosLds l = sc_pos_lds(a);
        if (l.wlds) hipLaunchKernelGGL(k_sc_bwd_pos<true>, dim3(static_cast<unsigned>(g.Gp)), dim3(kScNT), sizeof(float) * l.total, st, a, p, l);
        else hipLaunchKernelGGL(k_sc_bwd_pos<false>, dim3(static_cast<unsigned>(g.Gp)), dim3(kScNT), sizeof(float) * l.total, st, a, p, l);
        RECON_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_sc_reduce, dim3(static_cast<unsigned>(ceil_div64(g.slab + g.cells, kScNT))), dim3(kScNT), 0, st, a, p, r);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}
