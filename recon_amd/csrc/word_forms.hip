// E19 — the distinct word forms of a stage-B entity-context batch (recon_amd/word_forms.py).
// `get_char_indices` (utils/context_utils.py:265-283) lays every word slot of a context line out as [cfs - 1 pads][max_char_len ids]
// [cfs - 1 pads]; the char-CNN feature of a slot (models/models.py:57-61) depends on that window alone, so it is computed once per
// distinct window (a "form") and copied to the form's slots.  The copy is recon_pair_groups_expand (a row gather by slot_form); this
// file holds its backward: g_rows[f][:] = the sum of g_out[s][:] over the slots s of form f, form_slots[form_ptr[f] .. form_ptr[f + 1])
// in list order.  A segment can hold most of the batch (the all-PAD form), so it is cut into pieces of kWfPiece slots:
//
// k_wf_pieces: one wave per (piece id, chunk of 64 columns).  Form f owns the piece ids [base(f), base(f + 1)) with
//   base(f) = form_ptr[f] / kWfPiece + f, which is strictly ascending and leaves every form at least ceil(n_f / kWfPiece) ids
//   (floor(b / K) - floor(a / K) + 1 >= ceil((b - a) / K)), so no scan of the piece counts is needed: a wave finds its form by a binary
//   search of form_ptr, and the ids a form does not use leave at once.  Piece j of form f covers the slots form_ptr[f] + j kWfPiece ..
//   of ITS segment: the cut depends on the segment's length alone, never on the grid or on the other forms.  The wave reads 64 slot
//   numbers at a time and adds their rows in list order, eight loads in flight: one fp32 chain per element.
// k_wf_combine: one wave per (form, chunk of 64 columns) adds the form's piece sums in piece order; a form without a slot gets zeros.
// No atomics; nothing is destroyed (any number of backwards per forward, the same bits each time).  Everything read back from memory is
// clamped into its range before it is used as an address.
#include "recon_common.h"

namespace recon {
namespace {

constexpr int kWfPiece = 512;                         // slots per piece
constexpr int kWfThreads = 256;
constexpr int kWfUnroll = 8;                          // rows in flight per wave
constexpr int64_t kWfMaxCells = (int64_t{1} << 31) - 4096;      // of g_out and of g_rows: flat indices fit an int32 with room to spare

__device__ __forceinline__ int32_t wf_ptr(const int32_t* __restrict__ form_ptr, int32_t f, int32_t n_slots) { return min(max(form_ptr[f], 0), n_slots); }

__global__ void __launch_bounds__(kWfThreads) k_wf_pieces(const float* __restrict__ g_out, const int32_t* __restrict__ form_ptr,
                                                          const int32_t* __restrict__ form_slots, int32_t n_slots, int32_t S_d, int32_t F, int32_t chunks,
                                                          int32_t n_ids, float* __restrict__ partial) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t w = static_cast<int64_t>(blockIdx.x) * (kWfThreads / kWave) + (threadIdx.x >> 6);
    if (w >= static_cast<int64_t>(n_ids) * chunks) return;                  // (whole waves leave)
    const int32_t q = static_cast<int32_t>(w / chunks), chunk = static_cast<int32_t>(w - static_cast<int64_t>(q) * chunks);
    int32_t lo = 0, hi = S_d - 1;                                           // the last form whose base is at or below q
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (wf_ptr(form_ptr, mid, n_slots) / kWfPiece + mid <= q) lo = mid; else hi = mid - 1;
    }
    const int32_t f = lo;
    const int32_t a = wf_ptr(form_ptr, f, n_slots), b = max(a, wf_ptr(form_ptr, f + 1, n_slots));
    const int64_t j = static_cast<int64_t>(q) - (a / kWfPiece + f);
    if (j < 0) return;
    const int64_t start64 = a + j * kWfPiece;
    if (start64 >= b) return;                                               // an id the form does not use
    const int32_t start = static_cast<int32_t>(start64), end = min(start + kWfPiece, b);
    const int32_t col = chunk * kWave + lane;
    const bool live = col < F;
    float acc = 0.f;
    for (int32_t i0 = start; i0 < end; i0 += kWave) {
        const int32_t cnt = min(kWave, end - i0);
        const int32_t mine = lane < cnt ? min(max(form_slots[i0 + lane], 0), n_slots - 1) : 0;
        for (int32_t k = 0; k < cnt; k += kWfUnroll) {
            float x[kWfUnroll];
#pragma unroll
            for (int u = 0; u < kWfUnroll; ++u) {
                const int32_t s = __shfl(mine, min(k + u, kWave - 1), kWave);
                x[u] = (live && k + u < cnt) ? g_out[static_cast<int64_t>(s) * F + col] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kWfUnroll; ++u)
                if (k + u < cnt) acc += x[u];
        }
    }
    if (live) partial[static_cast<int64_t>(q) * F + col] = acc;
}

__global__ void __launch_bounds__(kWfThreads) k_wf_combine(const float* __restrict__ partial, const int32_t* __restrict__ form_ptr, int32_t n_slots, int32_t S_d,
                                                           int32_t F, int32_t chunks, int32_t n_ids, float* __restrict__ g_rows) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t w = static_cast<int64_t>(blockIdx.x) * (kWfThreads / kWave) + (threadIdx.x >> 6);
    if (w >= static_cast<int64_t>(S_d) * chunks) return;
    const int32_t f = static_cast<int32_t>(w / chunks), chunk = static_cast<int32_t>(w - static_cast<int64_t>(f) * chunks);
    const int32_t col = chunk * kWave + lane;
    if (col >= F) return;
    const int32_t a = wf_ptr(form_ptr, f, n_slots), b = max(a, wf_ptr(form_ptr, f + 1, n_slots));
    const int32_t pieces = (b - a + kWfPiece - 1) / kWfPiece;
    const int64_t base = a / kWfPiece + f;
    float acc = 0.f;
    for (int32_t j = 0; j < pieces; j += kWfUnroll) {
        float x[kWfUnroll];
#pragma unroll
        for (int u = 0; u < kWfUnroll; ++u) x[u] = j + u < pieces ? partial[min(base + j + u, static_cast<int64_t>(n_ids) - 1) * F + col] : 0.f;
#pragma unroll
        for (int u = 0; u < kWfUnroll; ++u)
            if (j + u < pieces) acc += x[u];
    }
    g_rows[static_cast<int64_t>(f) * F + col] = acc;
}

bool wf_shape_ok(int64_t n_slots, int64_t S_d, int64_t F) {
    return n_slots >= 0 && S_d >= 0 && F >= 1 && n_slots * F < kWfMaxCells && S_d * F < kWfMaxCells && (n_slots / kWfPiece + S_d + 1) * F < kWfMaxCells;
}

}  // namespace
}  // namespace recon

extern "C" int32_t recon_word_forms_piece(void) { return recon::kWfPiece; }

extern "C" size_t recon_word_forms_reduce_workspace_bytes(int64_t n_slots, int64_t S_d, int32_t F) {
    if (!recon::wf_shape_ok(n_slots, S_d, F)) return 0;
    return align_up(static_cast<size_t>((n_slots / recon::kWfPiece + S_d + 1) * F) * sizeof(float), 16);
}

extern "C" int recon_word_forms_reduce(const float* g_out, const int32_t* form_ptr, const int32_t* form_slots, int64_t n_slots, int64_t S_d, int32_t F,
                                       float* g_rows, void* workspace, size_t workspace_bytes, recon_stream_t stream) {
    using namespace recon;
    if (n_slots < 0 || S_d < 0 || F < 1) return RECON_ERR_INVALID;
    if (S_d > 0 && (!form_ptr || !g_rows || !workspace)) return RECON_ERR_INVALID;
    if (n_slots > 0 && S_d > 0 && (!g_out || !form_slots)) return RECON_ERR_INVALID;
    if (!wf_shape_ok(n_slots, S_d, F)) return RECON_ERR_UNSUPPORTED;
    if (S_d == 0) return RECON_OK;
    if (reinterpret_cast<uintptr_t>(workspace) % 4) return RECON_ERR_INVALID;
    if (workspace_bytes < recon_word_forms_reduce_workspace_bytes(n_slots, S_d, F)) return RECON_ERR_WORKSPACE;
    const int32_t n = static_cast<int32_t>(n_slots), s = static_cast<int32_t>(S_d);
    const int32_t n_ids = static_cast<int32_t>(n_slots / kWfPiece + S_d + 1);
    const int32_t chunks = (F + kWave - 1) / kWave;
    constexpr int kWaves = kWfThreads / kWave;
    float* partial = static_cast<float*>(workspace);
    if (n_slots > 0) {
        hipLaunchKernelGGL(k_wf_pieces, dim3(static_cast<unsigned>(ceil_div64(static_cast<int64_t>(n_ids) * chunks, kWaves))), dim3(kWfThreads), 0,
                           as_stream(stream), g_out, form_ptr, form_slots, n, s, F, chunks, n_ids, partial);
        RECON_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_wf_combine, dim3(static_cast<unsigned>(ceil_div64(S_d * chunks, kWaves))), dim3(kWfThreads), 0, as_stream(stream), partial, form_ptr,
                       n, s, F, chunks, n_ids, g_rows);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}
