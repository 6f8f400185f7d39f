// E12 — the entity-level tail of the entity-context encoder (models/models.py:73-81): conv1d_entity over the line states, the line mask
// and the max over the lines, without the [U][E][P] convolution output or its masked copy:
//     out[u][e] = max over unmasked p of  bias[e] + sum_{j < k} sum_c weight[e][c][j] states[u][p + j][c],      P = Ln - k + 1 positions
// with the lowest position on an exact tie, -inf for an entity without an unmasked position and NaN where an unmasked position is NaN.
// The winning position is kept as one byte per output (255: none), which is all the backward needs:
//     d_states[u][l][c] = sum_{e asc} [0 <= l - pos[u][e] < k] g[u][e] weight[e][c][l - pos[u][e]]
//     d_weight[e][c][j] = sum_u g[u][e] states[u][pos[u][e] + j][c]          d_bias[e] = sum_u [pos[u][e] != 255] g[u][e]
// Everything is fp32 on the VALU, no atomics, every sum in an order the shapes alone decide.
//
// Why the VALU and not v_mfma_f32_16x16x4_f32: E = 8 fills half of a 16-wide tile, the product is 23 MFLOP at the reference's shape
// (450 x 32 x 100 -> 8) and both forms are exact fp32 fma chains at the same rate; what the kernels cost is their launches and the one
// read of the states.  The VALU form takes any (C, E, k) without padding a fragment.
//
// k_lp_fwd: one workgroup per entity.  The reduction index r = j C + c (k C values) is cut into chunks of RC, the positions into chunks
//   of PC; a chunk's weight rows [E][RC] and its position rows [PC][RC] (row p is the k line states under position p, side by side: for
//   k = 1 the line state itself) sit in LDS at the odd pitch RC + 1, so that the E weight rows and the PC position rows a wave reads in one
//   instruction fall on different banks.  A thread owns up to 4 cells (p, e) of a position chunk, e fastest: one fma chain per cell in r
//   order, started at 0, the bias added last.  At the reference's widths PC = P = 32 and RC = 100: one chunk, one cell per thread.  The
//   values go through LDS to thread e, which walks the chunk's positions upwards and keeps the first maximum among the unmasked ones.
// k_lp_bwd: workgroup z takes the entities [z per, (z + 1) per), per = ceil(U / min(256, U)): a function of U alone.  It walks them
//   upwards, 16 at a time, their g_out and positions staged in LDS.  For each entity it writes every cell of the entity's d_states rows
//   once (zeros included: the host hands uninitialised memory; the weight is staged in LDS where it fits 32 KiB, and the channels e
//   are then tried by selects, so that their LDS reads go out together), and it adds the entity to its slab [E][C k + 1] of
//   (d_weight | d_bias), held in registers: a thread owns up to 4 slab cells per pass, an absent position is a select, not a branch,
//   so the loads of the winning line states do not wait for one another.  A slab of more than 1024 cells takes further passes over
//   the group's entities.  The slab goes to the workspace.  Either half is skipped when its result is not wanted.
// k_lp_reduce: adds the slabs in group order.
//
// The ragged form (recon_line_pool_ragged_*): the states are a flat [L][C] list and entity u owns the rows line_ptr[u] .. line_ptr[u + 1]
//   (recon_amd.RaggedLines), every one of them present: P_u = n_u - k + 1 positions, none masked, -inf and byte 255 where n_u < k.  The
//   same two kernel bodies, instantiated with RAGGED: the row base and the position count come from line_ptr instead of u Ln and the
//   mask; chunk sizes come from the longest entity, and a sum's order does not depend on them (one fma chain in r order per cell), so an
//   entity gives the bits the padded form gives for it.  The entity groups of the backward are those of the padded form.
#include "recon_common.h"

#include <cmath>

namespace recon {
namespace {

constexpr int kLpThreads = 256;
constexpr int kLpAcc = 4;                            // cells per thread and pass
constexpr int kLpCells = kLpThreads * kLpAcc;
constexpr int kLpMaxGroups = 256;                    // MAX_ENTITY_GROUPS of recon_amd/line_pool.py
constexpr int kLpLdsFloats = 12288;                  // 48 KiB for the two staged tiles of k_lp_fwd
constexpr int kLpMaxP = 255, kLpMaxR = 1024, kLpMaxE = 64;
constexpr int kLpNone = 255;                         // the position byte of an output without an unmasked position
constexpr int kLpBwdChunk = 16;                      // entities whose g_out and positions k_lp_bwd holds in LDS at a time
constexpr int kLpBwdWeightFloats = 8192;             // the largest weight k_lp_bwd stages (32 KiB)

struct LpTiles { int32_t PC, RC; };
// the forward's chunk sizes: up to 1024 cells per position chunk, then the longest reduction chunk whose two tiles fit the LDS budget
inline LpTiles lp_tiles(int P, int R, int E) {
    LpTiles t;
    t.PC = P < kLpCells / E ? P : kLpCells / E;
    const int rc = kLpLdsFloats / (E + t.PC) - 1;
    t.RC = R < rc ? R : rc;
    return t;
}
inline int64_t lp_per(int64_t U) { return ceil_div64(U, U < kLpMaxGroups ? U : kLpMaxGroups); }
inline int64_t lp_groups(int64_t U) { return ceil_div64(U, lp_per(U)); }

// RAGGED: `rows` is line_ptr [U + 1] and every position of an entity is unmasked; otherwise `rows` is the mask [U][P] and Ln the line count
template <bool RAGGED>
__global__ void __launch_bounds__(kLpThreads) k_lp_fwd(const float* __restrict__ states, int64_t ld, const float* __restrict__ weight,
                                                       const float* __restrict__ bias, const void* __restrict__ rows, int32_t Ln, int32_t C,
                                                       int32_t E, int32_t k, int32_t PC, int32_t RC, float* __restrict__ out,
                                                       uint8_t* __restrict__ pos) {
    extern __shared__ __align__(16) float lp_lds[];
    __shared__ float vals[kLpCells];
    __shared__ uint8_t masked[kLpMaxP + 1];
    const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const int64_t u = blockIdx.x;
    const int R = C * k, pitch = RC + 1;
    int P;
    int64_t row0;
    if constexpr (RAGGED) {
        const int32_t* line_ptr = static_cast<const int32_t*>(rows);
        row0 = line_ptr[u];
        P = min(line_ptr[u + 1] - static_cast<int32_t>(row0) - k + 1, kLpMaxP);      // <= 0: an entity shorter than the filter
    } else {
        row0 = u * Ln;
        P = Ln - k + 1;
        if (t < P) masked[t] = static_cast<const uint8_t*>(rows)[u * P + t];
    }
    float* Ws = lp_lds;
    float* Xs = lp_lds + E * pitch;
    const float* srow = states + row0 * ld;
    float best = -INFINITY;                                              // thread e < E: the maximum so far and where
    int at = kLpNone;
    for (int p0 = 0; p0 < P; p0 += PC) {
        const int pcn = min(PC, P - p0), ncell = pcn * E;
        int pp[kLpAcc], ee[kLpAcc];
        float acc[kLpAcc], bv[kLpAcc];
#pragma unroll
        for (int a = 0; a < kLpAcc; ++a) {
            const int q = t + a * kLpThreads, qq = q < ncell ? q : 0;
            pp[a] = qq / E;
            ee[a] = qq - pp[a] * E;
            acc[a] = 0.f;
            bv[a] = bias[ee[a]];                                         // (asked for here: it has arrived when the sums are done)
        }
        for (int r0 = 0; r0 < R; r0 += RC) {
            const int rcn = min(RC, R - r0);
            __syncthreads();                                             // the previous tiles and values have been read
            // a wave stages whole rows, lane = place in the row: no division per element (k = 1: r is the channel itself)
            if (p0 == 0 || RC < R) {                                     // (one reduction chunk: the weight stays where it is)
                for (int e = wv; e < E; e += kLpThreads / kWave) {
                    for (int rr = lane; rr < rcn; rr += kWave) {
                        const int r = r0 + rr, j = k == 1 ? 0 : r / C, c = r - j * C;
                        Ws[e * pitch + rr] = weight[e * R + c * k + j];
                    }
                }
            }
            for (int pi = wv; pi < pcn; pi += kLpThreads / kWave) {
                for (int rr = lane; rr < rcn; rr += kWave) {
                    const int r = r0 + rr, j = k == 1 ? 0 : r / C, c = r - j * C;
                    Xs[pi * pitch + rr] = srow[(p0 + pi + j) * ld + c];
                }
            }
            __syncthreads();
#pragma unroll
            for (int a = 0; a < kLpAcc; ++a) {
                if (a * kLpThreads < ncell) {                            // uniform
                    const float* x = Xs + pp[a] * pitch;
                    const float* w = Ws + ee[a] * pitch;
                    float s = acc[a];
#pragma unroll 8
                    for (int rr = 0; rr < rcn; ++rr) s = fmaf(x[rr], w[rr], s);
                    acc[a] = s;
                }
            }
        }
#pragma unroll
        for (int a = 0; a < kLpAcc; ++a) {
            const int q = t + a * kLpThreads;
            if (q < ncell) vals[q] = acc[a] + bv[a];
        }
        __syncthreads();
        if (t < E) {
#pragma unroll 4
            for (int pi = 0; pi < pcn; ++pi) {                           // (selects, not branches: the reads of the next positions go ahead)
                const float v = vals[pi * E + t];
                const bool take = (RAGGED || !masked[p0 + pi]) && (at == kLpNone || v > best || (v != v && best == best));
                best = take ? v : best;
                at = take ? p0 + pi : at;
            }
        }
    }
    if (t < E) {
        out[u * E + t] = best;
        if (pos) pos[u * E + t] = static_cast<uint8_t>(at);
    }
}

// WLDS: the weight (E C k <= kLpBwdWeightFloats) is staged in LDS for the d_states pass; otherwise it is read where it lies
// RAGGED: entity u's rows of states and g_states are line_ptr[u] .. line_ptr[u + 1] (g_states is [L][C]); otherwise u Ln .. (u + 1) Ln
template <bool WLDS, bool RAGGED>
__global__ void __launch_bounds__(kLpThreads) k_lp_bwd(const float* __restrict__ states, int64_t ld, const float* __restrict__ weight,
                                                       const float* __restrict__ g_out, const uint8_t* __restrict__ pos, int64_t U, int64_t per,
                                                       int32_t Ln, int32_t C, int32_t E, int32_t k, const int32_t* __restrict__ line_ptr,
                                                       float* __restrict__ g_states, float* __restrict__ slabs) {
    extern __shared__ __align__(16) float lp_w[];
    __shared__ float gs[kLpBwdChunk * kLpMaxE];                          // g_out and the positions of a chunk of entities
    __shared__ int ps[kLpBwdChunk * kLpMaxE];
    const int t = threadIdx.x;
    const int64_t z = blockIdx.x, u0 = z * per, u1 = min(U, u0 + per);
    const int R = C * k, slab = E * (R + 1);
    if constexpr (WLDS)
        if (g_states)
            for (int i = t; i < E * R; i += kLpThreads) lp_w[i] = weight[i];
    const float* w = WLDS ? lp_w : weight;
    float* mine = slabs ? slabs + z * slab : nullptr;
    // a pass accumulates up to 1024 slab cells over all entities of the group; the first pass also writes the entities' d_states rows
    for (int q0 = 0; q0 < (slabs ? slab : 1); q0 += kLpCells) {
        int ee[kLpAcc], cc[kLpAcc], jj[kLpAcc];
        bool ok[kLpAcc], isb[kLpAcc];
        float acc[kLpAcc];
#pragma unroll
        for (int a = 0; a < kLpAcc; ++a) {
            const int q = q0 + t + a * kLpThreads;
            ok[a] = slabs && q < slab;
            const int qq = ok[a] ? q : 0;
            ee[a] = qq / (R + 1);
            const int r = qq - ee[a] * (R + 1);                          // the weight's own order: r = c k + j; r == R: the bias cell
            isb[a] = r == R;
            cc[a] = isb[a] ? 0 : r / k;
            jj[a] = isb[a] ? 0 : r - cc[a] * k;
            acc[a] = 0.f;
        }
        for (int64_t uc = u0; uc < u1; uc += kLpBwdChunk) {              // a chunk's g_out and positions through LDS: no load waits for another
            const int n = static_cast<int>(min(static_cast<int64_t>(kLpBwdChunk), u1 - uc));
            __syncthreads();
            for (int i = t; i < n * E; i += kLpThreads) {
                gs[i] = g_out[uc * E + i];
                ps[i] = pos[uc * E + i];
            }
            __syncthreads();
            if (g_states && q0 == 0) {
                for (int uu = 0; uu < n; ++uu) {
                    const int64_t row0 = RAGGED ? line_ptr[uc + uu] : (uc + uu) * Ln;
                    const int cells = (RAGGED ? line_ptr[uc + uu + 1] - static_cast<int32_t>(row0) : Ln) * C;
                    float* drow = g_states + row0 * C;
                    const float* gu = gs + uu * E;
                    const int* pu = ps + uu * E;
                    for (int i = t; i < cells; i += kLpThreads) {
                        const int l = i / C, c = i - l * C;
                        float s = 0.f;
                        if constexpr (WLDS) {                            // selects: the LDS reads of the channels e go out together
#pragma unroll 8
                            for (int e = 0; e < E; ++e) {
                                const int p = pu[e], j = l - p;
                                const bool hit = p != kLpNone && j >= 0 && j < k;
                                const float wv = w[e * R + c * k + (hit ? j : 0)];
                                s = hit ? fmaf(gu[e], wv, s) : s;
                            }
                        } else {
                            for (int e = 0; e < E; ++e) {
                                const int p = pu[e], j = l - p;
                                if (p != kLpNone && j >= 0 && j < k) s = fmaf(gu[e], w[e * R + c * k + j], s);
                            }
                        }
                        drow[i] = s;
                    }
                }
            }
            if (slabs) {
                for (int uu = 0; uu < n; ++uu) {
                    const int64_t row0 = RAGGED ? line_ptr[uc + uu] : (uc + uu) * Ln;
#pragma unroll
                    for (int a = 0; a < kLpAcc; ++a) {
                        const int p = ps[uu * E + ee[a]];
                        const bool valid = ok[a] && p != kLpNone;        // (an absent position reads line 0 and is not added)
                        float x;
                        if constexpr (RAGGED) x = valid ? states[(row0 + p + jj[a]) * ld + cc[a]] : 0.f;      // (an entity may own no line: no read)
                        else x = states[(row0 + (valid ? p : 0) + jj[a]) * ld + cc[a]];
                        acc[a] = valid ? fmaf(gs[uu * E + ee[a]], isb[a] ? 1.f : x, acc[a]) : acc[a];
                    }
                }
            }
        }
#pragma unroll
        for (int a = 0; a < kLpAcc; ++a)
            if (ok[a]) mine[q0 + t + a * kLpThreads] = acc[a];
    }
}

__global__ void __launch_bounds__(kLpThreads) k_lp_reduce(const float* __restrict__ slabs, int32_t G, int32_t slab, int32_t R,
                                                          float* __restrict__ g_w, float* __restrict__ g_b) {
    const int q = blockIdx.x * kLpThreads + threadIdx.x;
    if (q >= slab) return;
    float s = 0.f;
#pragma unroll 16
    for (int z = 0; z < G; ++z) s += slabs[static_cast<int64_t>(z) * slab + q];
    const int e = q / (R + 1), r = q - e * (R + 1);
    if (r < R) {
        if (g_w) g_w[e * R + r] = s;
    } else if (g_b) {
        g_b[e] = s;
    }
}

bool lp_shape_ok(int64_t U, int32_t Ln, int32_t C, int32_t E, int32_t k) {
    if (U < 0 || U > (int64_t{1} << 30) || Ln < 1 || C < 1 || E < 1 || E > kLpMaxE || k < 1 || k > Ln) return false;
    return Ln - k + 1 <= kLpMaxP && static_cast<int64_t>(C) * k <= kLpMaxR;
}


// the ragged form: U entities over L rows, the longest of n_max; an entity may own no row and may be shorter than the filter
bool lp_ragged_ok(int64_t U, int64_t L, int32_t n_max, int32_t C, int32_t E, int32_t k) {
    if (U < 0 || U > (int64_t{1} << 30) || L < 0 || L >= (int64_t{1} << 31) || n_max < 0 || n_max > L || L > U * n_max) return false;
    if (C < 1 || E < 1 || E > kLpMaxE || k < 1) return false;
    return n_max - k + 1 <= kLpMaxP && static_cast<int64_t>(C) * k <= kLpMaxR;
}

// the forward of either form: `rows` is the mask [U][P] of Ln lines per entity, or line_ptr [U + 1] with Ln = the longest entity's lines
template <bool RAGGED>
int lp_run_fwd(const float* states, int64_t ld, const float* weight, const float* bias, const void* rows, int64_t U, int32_t Ln, int32_t C, int32_t E,
               int32_t k, float* out, void* positions, recon_stream_t stream) {
    const LpTiles tl = lp_tiles(Ln - k + 1 > 1 ? Ln - k + 1 : 1, C * k, E);
    const size_t lds = static_cast<size_t>(E + tl.PC) * (tl.RC + 1) * sizeof(float);
    hipLaunchKernelGGL(k_lp_fwd<RAGGED>, dim3(static_cast<unsigned>(U)), dim3(kLpThreads), lds, as_stream(stream), states, ld, weight, bias, rows, Ln, C,
                       E, k, tl.PC, tl.RC, out, static_cast<uint8_t*>(positions));
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

// the backward of either form behind the argument checks; workspace: lp_groups(U) slabs
template <bool RAGGED>
int lp_run_bwd(const float* states, int64_t ld, const float* weight, const float* g_out, const void* positions, const int32_t* line_ptr, int64_t U,
               int32_t Ln, int32_t C, int32_t E, int32_t k, float* g_states, float* g_w, float* g_b, void* workspace, recon_stream_t stream) {
    hipStream_t st = as_stream(stream);
    const bool params = g_w || g_b;
    const int R = C * k, slab = E * (R + 1);
    const int64_t G = lp_groups(U);
    float* slabs = params ? static_cast<float*>(workspace) : nullptr;
    const uint8_t* pb = static_cast<const uint8_t*>(positions);
    if (g_states && E * R <= kLpBwdWeightFloats)
        hipLaunchKernelGGL((k_lp_bwd<true, RAGGED>), dim3(static_cast<unsigned>(G)), dim3(kLpThreads), sizeof(float) * E * R, st, states, ld, weight, g_out,
                           pb, U, lp_per(U), Ln, C, E, k, line_ptr, g_states, slabs);
    else
        hipLaunchKernelGGL((k_lp_bwd<false, RAGGED>), dim3(static_cast<unsigned>(G)), dim3(kLpThreads), 0, st, states, ld, weight, g_out, pb, U, lp_per(U),
                           Ln, C, E, k, line_ptr, g_states, slabs);
    RECON_CHECK_LAUNCH();
    if (params) {
        hipLaunchKernelGGL(k_lp_reduce, dim3(static_cast<unsigned>((slab + kLpThreads - 1) / kLpThreads)), dim3(kLpThreads), 0, st, slabs,
                           static_cast<int32_t>(G), slab, R, g_w, g_b);
        RECON_CHECK_LAUNCH();
    }
    return RECON_OK;
}

// zeros in every wanted parameter gradient of a call without an entity, no kernel
int lp_zero_params(float* g_w, float* g_b, int32_t E, int32_t R, hipStream_t st) {
    if (g_w && hipMemsetAsync(g_w, 0, sizeof(float) * E * R, st) != hipSuccess) return RECON_ERR_LAUNCH;
    if (g_b && hipMemsetAsync(g_b, 0, sizeof(float) * E, st) != hipSuccess) return RECON_ERR_LAUNCH;
    return RECON_OK;
}

}  // namespace
}  // namespace recon

extern "C" int recon_line_pool_supported(int64_t U, int32_t Ln, int32_t C, int32_t E, int32_t k) { return recon::lp_shape_ok(U, Ln, C, E, k) ? 1 : 0; }

extern "C" size_t recon_line_pool_workspace_bytes(int64_t U, int32_t Ln, int32_t C, int32_t E, int32_t k) {
    using namespace recon;
    if (!lp_shape_ok(U, Ln, C, E, k) || U == 0) return 0;
    return align_up(static_cast<size_t>(lp_groups(U)) * E * (C * k + 1) * sizeof(float), 16);
}

extern "C" int recon_line_pool_fwd(const float* states, int64_t ld, const float* weight, const float* bias, const void* mask, int64_t U, int32_t Ln,
                                   int32_t C, int32_t E, int32_t k, float* out, void* positions, recon_stream_t stream) {
    using namespace recon;
    if (U < 0 || Ln < 1 || C < 1 || E < 1 || k < 1 || k > Ln) return RECON_ERR_INVALID;
    if (!lp_shape_ok(U, Ln, C, E, k)) return RECON_ERR_UNSUPPORTED;
    if (U == 0) return RECON_OK;
    if (!states || !weight || !bias || !mask || !out || ld < C) return RECON_ERR_INVALID;
    return lp_run_fwd<false>(states, ld, weight, bias, mask, U, Ln, C, E, k, out, positions, stream);
}

extern "C" int recon_line_pool_bwd(const float* states, int64_t ld, const float* weight, const float* g_out, const void* positions, int64_t U,
                                   int32_t Ln, int32_t C, int32_t E, int32_t k, float* g_states, float* g_w, float* g_b, void* workspace,
                                   size_t workspace_bytes, recon_stream_t stream) {
    using namespace recon;
    if (U < 0 || Ln < 1 || C < 1 || E < 1 || k < 1 || k > Ln) return RECON_ERR_INVALID;
    if (!lp_shape_ok(U, Ln, C, E, k)) return RECON_ERR_UNSUPPORTED;
    const bool params = g_w || g_b;
    if (U == 0) return lp_zero_params(g_w, g_b, E, C * k, as_stream(stream));
    if (!g_states && !params) return RECON_OK;
    if (!states || !weight || !g_out || !positions || ld < C) return RECON_ERR_INVALID;
    if (params) {
        if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return RECON_ERR_INVALID;
        if (workspace_bytes < recon_line_pool_workspace_bytes(U, Ln, C, E, k)) return RECON_ERR_WORKSPACE;
    }
    return lp_run_bwd<false>(states, ld, weight, g_out, positions, nullptr, U, Ln, C, E, k, g_states, g_w, g_b, workspace, stream);
}

extern "C" int recon_line_pool_ragged_supported(int64_t U, int64_t L, int32_t n_max, int32_t C, int32_t E, int32_t k) {
    return recon::lp_ragged_ok(U, L, n_max, C, E, k) ? 1 : 0;
}

extern "C" size_t recon_line_pool_ragged_workspace_bytes(int64_t U, int64_t L, int32_t n_max, int32_t C, int32_t E, int32_t k) {
    using namespace recon;
    if (!lp_ragged_ok(U, L, n_max, C, E, k) || U == 0) return 0;
    return align_up(static_cast<size_t>(lp_groups(U)) * E * (C * k + 1) * sizeof(float), 16);
}

extern "C" int recon_line_pool_ragged_fwd(const float* states, int64_t ld, const float* weight, const float* bias, const int32_t* line_ptr, int64_t U,
                                          int64_t L, int32_t n_max, int32_t C, int32_t E, int32_t k, float* out, void* positions,
                                          recon_stream_t stream) {
    using namespace recon;
    if (U < 0 || L < 0 || n_max < 0 || C < 1 || E < 1 || k < 1) return RECON_ERR_INVALID;
    if (!lp_ragged_ok(U, L, n_max, C, E, k)) return RECON_ERR_UNSUPPORTED;
    if (U == 0) return RECON_OK;
    if ((!states && L > 0) || !weight || !bias || !line_ptr || !out || ld < C) return RECON_ERR_INVALID;
    return lp_run_fwd<true>(states, ld, weight, bias, line_ptr, U, n_max, C, E, k, out, positions, stream);
}

extern "C" int recon_line_pool_ragged_bwd(const float* states, int64_t ld, const float* weight, const float* g_out, const void* positions,
                                          const int32_t* line_ptr, int64_t U, int64_t L, int32_t n_max, int32_t C, int32_t E, int32_t k,
                                          float* g_states, float* g_w, float* g_b, void* workspace, size_t workspace_bytes, recon_stream_t stream) {
    using namespace recon;
    if (U < 0 || L < 0 || n_max < 0 || C < 1 || E < 1 || k < 1) return RECON_ERR_INVALID;
    if (!lp_ragged_ok(U, L, n_max, C, E, k)) return RECON_ERR_UNSUPPORTED;
    const bool params = g_w || g_b;
    if (U == 0) return lp_zero_params(g_w, g_b, E, C * k, as_stream(stream));
    if (L == 0) g_states = nullptr;                                      // no row: nothing to write
    if (!g_states && !params) return RECON_OK;
    if ((!states && L > 0) || !weight || !g_out || !positions || !line_ptr || ld < C) return RECON_ERR_INVALID;
    if (params) {
        if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return RECON_ERR_INVALID;
        if (workspace_bytes < recon_line_pool_ragged_workspace_bytes(U, L, n_max, C, E, k)) return RECON_ERR_WORKSPACE;
    }
    return lp_run_bwd<true>(states, ld, weight, g_out, positions, line_ptr, U, n_max, C, E, k, g_states, g_w, g_b, workspace, stream);
}
