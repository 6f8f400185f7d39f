// E18 — the distinct (sentence, pair markers) sequences of a stage-B batch (recon_amd/pair_groups.py).
// `to_indices_with_real_entities_and_entity_nums_with_vertex_padding` (parsing/legacy_sp_models.py:294-326) fills a marker row only for the
// pairs a sentence has and `GPGNN.encode` (models/models.py:160-184) copies the sentence once per pair slot, so the slots of a sentence
// whose marker rows are equal are the same LSTM input.  Two pair slots of ONE sentence share a sequence exactly when their marker rows
// are equal element by element; the representative of a group is its lowest c; the distinct sequences are numbered in (b, lowest c) order.
// Selection, ordering and copying only; no atomics on global memory, every output the same bits from run to run.
//
// k_pg_local: one workgroup of 256 threads per sentence, thread c owns slot c (C <= 256).  A row is compared as `words` machine words of
//   the widest size (8, 4, 2 or 1 bytes) that divides both the row's byte length and the array's address: the comparison is exact whatever
//   the element type, and there is no hash, hence no collision case.  The sentence's rows are staged in LDS first (up to 48 KiB; read in
//   place above).  Thread c walks c' = 0 .. c - 1 and stops at the first equal row (first[c] = c', else c).  The representatives' flags go
//   to LDS; lrank[c] = the number of representatives below first[c], the group's number inside the sentence; counts[b] = the sentence's
//   distinct rows.
// k_pg_scan: ONE workgroup of 1024 threads scans counts in b order (k_cb_scan's scheme: a thread owns ceil(B / 1024) <= 8 consecutive
//   sentences, a wave scans by __shfl_up, thread 0 the 16 wave totals) into seq_ptr [B + 1]; then pair_seq[p] = seq_ptr[b] + lrank[p],
//   seq_pair[j] = p for a representative, and the representatives' rows of `sentence` and `markers` as sentence_d [S_d][T] and
//   markers_d [S_d][T] in the caller's index type.  Everything read back from memory (first, lrank, counts, seq_pair) is clamped into its
//   range before it is used as an address; with a scanned total other than the caller's the status word is set, pair_seq is clamped
//   below `total`, the rows from the scanned total up to `total` are zeros and no row at or behind `total` is written.  total < 0: seq_ptr
//   and pair_seq alone (the host reads seq_ptr[B]).
// k_pg_expand: out[p][:] = rows[pair_seq[p]][:], one 16-byte store per thread (element stores where F is no multiple of 4 or a base is
//   unaligned).
// k_pg_reduce: g_rows[j][:] = the sum over the slots c of j's sentence with pair_seq[b C + c] = j of g_out[b C + c][:], c ascending: one
//   wave per (sequence, chunk of 64 vectors); the wave reads 64 slots' pair_seq at a time and walks the ballot's set bits in order: one
//   fp32 chain per element, no atomics, nothing destroyed.
#include "recon_common.h"

namespace recon {
namespace {

constexpr int kPgMaxC = 256;                          // one thread per slot of a sentence
constexpr int kPgMaxB = 8192;                         // k_pg_scan: 1024 threads x 8 sentences
constexpr int kPgScanThreads = 1024;
constexpr int kPgThreads = 256;
constexpr int64_t kPgMaxCells = (int64_t{1} << 31) - 4096;      // of markers, and of an expanded block: flat indices are int32

template <typename WT, bool LDS>
__global__ void __launch_bounds__(kPgMaxC) k_pg_local(const WT* __restrict__ rows, int32_t words, int32_t C, int32_t* __restrict__ first,
                                                      int32_t* __restrict__ lrank, int32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pg_sm[];
    __shared__ int32_t rep[kPgMaxC];
    const int c = threadIdx.x;
    const int64_t b = blockIdx.x;
    const WT* mine_rows = rows + b * C * words;                     // the sentence's C rows
    if constexpr (LDS) {                                             // staged once: every row is compared with up to C - 1 others
        WT* staged = reinterpret_cast<WT*>(pg_sm);
        for (int i = c; i < C * words; i += kPgMaxC) staged[i] = mine_rows[i];
        __syncthreads();
        mine_rows = staged;
    }
    int32_t f = c;
    if (c < C) {
        const WT* mine = mine_rows + c * words;
        for (int o = 0; o < c; ++o) {
            const WT* other = mine_rows + o * words;
            int w = 0;
            while (w < words && mine[w] == other[w]) ++w;
            if (w == words) { f = o; break; }
        }
    }
    rep[c] = (c < C && f == c) ? 1 : 0;
    __syncthreads();
    if (c < C) {
        int32_t r = 0;
        for (int o = 0; o < f; ++o) r += rep[o];
        first[b * C + c] = f;
        lrank[b * C + c] = r;
    }
    if (c == 0) {
        int32_t n = 0;
        for (int o = 0; o < C; ++o) n += rep[o];
        counts[b] = n;
    }
}

template <typename ST, typename MT, typename OT>
__global__ void __launch_bounds__(kPgScanThreads) k_pg_scan(const ST* __restrict__ sentence, const MT* __restrict__ markers, const int32_t* __restrict__ first,
                                                            const int32_t* __restrict__ lrank, const int32_t* __restrict__ counts, int32_t B, int32_t C,
                                                            int32_t T, int32_t total, int32_t* __restrict__ seq_pair, int32_t* __restrict__ pair_seq,
                                                            int32_t* __restrict__ seq_ptr, OT* __restrict__ sentence_d, OT* __restrict__ markers_d,
                                                            int32_t* __restrict__ status) {
    __shared__ uint32_t wsum[kPgScanThreads / kWave];
    __shared__ int32_t ptr[kPgMaxB + 1];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int per = (B + kPgScanThreads - 1) / kPgScanThreads;
    const int b0 = min(B, tid * per), b1 = min(B, b0 + per);
    uint32_t sum = 0;
    for (int b = b0; b < b1; ++b) sum += static_cast<uint32_t>(min(max(counts[b], 0), C));
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += o;
    }
    if (lane == kWave - 1) wsum[wv] = incl;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int w = 0; w < kPgScanThreads / kWave; ++w) { const uint32_t s = wsum[w]; wsum[w] = run; run += s; }
        ptr[B] = static_cast<int32_t>(run);
    }
    __syncthreads();
    int32_t base = static_cast<int32_t>(wsum[wv] + incl - sum);
    for (int b = b0; b < b1; ++b) {
        ptr[b] = base;
        base += min(max(counts[b], 0), C);
    }
    __syncthreads();
    const int32_t scanned = ptr[B];
    for (int b = tid; b <= B; b += kPgScanThreads) seq_ptr[b] = ptr[b];
    const bool count_only = total < 0;
    if (tid == 0 && !count_only && scanned != total) status[0] = 1;
    const int32_t cap = count_only ? scanned : total;                       // rows that exist for the caller
    const int32_t n_pairs = B * C;
    for (int32_t p = tid; p < n_pairs; p += kPgScanThreads) {
        const int32_t b = p / C, c = p - b * C;
        const int32_t f = min(max(first[p], 0), c);
        const int32_t r = min(max(lrank[p], 0), C - 1);
        const int32_t j = ptr[b] + r;
        pair_seq[p] = min(j, max(cap - 1, 0));
        if (!count_only && f == c && j < cap) seq_pair[j] = p;
    }
    if (count_only) return;
    __syncthreads();                                                        // seq_pair: this workgroup's own stores, read back below
    const int32_t rows = min(scanned, cap);                                 // rows in [scanned, total) have no representative: zeros, so
    for (int32_t j = scanned + tid; j < cap; j += kPgScanThreads) seq_pair[j] = 0;       // that no later reader meets an unwritten index
    const int32_t cells = cap * T;
    constexpr int kUnroll = 4;                                              // four cells' loads in flight per thread: the copy is latency bound
    for (int32_t i0 = tid; i0 < cells; i0 += kUnroll * kPgScanThreads) {
        OT sv[kUnroll], mv[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int32_t i = min(i0 + u * kPgScanThreads, cells - 1);
            const int32_t j = i / T, t = i - j * T;
            const int32_t p = min(max(j < rows ? seq_pair[j] : 0, 0), n_pairs - 1);
            const int32_t b = p / C;
            sv[u] = j < rows ? static_cast<OT>(sentence[static_cast<int64_t>(b) * T + t]) : OT(0);
            mv[u] = j < rows ? static_cast<OT>(markers[static_cast<int64_t>(p) * T + t]) : OT(0);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int32_t i = i0 + u * kPgScanThreads;
            if (i < cells) { sentence_d[i] = sv[u]; markers_d[i] = mv[u]; }
        }
    }
}

template <int VEC>
__global__ void __launch_bounds__(kPgThreads) k_pg_expand(const float* __restrict__ rows, const int32_t* __restrict__ pair_seq, int32_t n_pairs, int32_t S_d,
                                                          int32_t F, float* __restrict__ out) {
    const int32_t fv = F / VEC;
    const int64_t v = static_cast<int64_t>(blockIdx.x) * kPgThreads + threadIdx.x;
    if (v >= static_cast<int64_t>(n_pairs) * fv) return;
    const int32_t p = static_cast<int32_t>(v / fv), k = static_cast<int32_t>(v - static_cast<int64_t>(p) * fv);
    const int32_t j = min(max(pair_seq[p], 0), S_d - 1);
    float x[VEC];
    load_vec<VEC>(x, rows + static_cast<int64_t>(j) * F + k * VEC);
    store_vec<VEC>(out + static_cast<int64_t>(p) * F + k * VEC, x);
}

template <int VEC>
__global__ void __launch_bounds__(kPgThreads) k_pg_reduce(const float* __restrict__ g_out, const int32_t* __restrict__ pair_seq, const int32_t* __restrict__ seq_pair,
                                                          int32_t B, int32_t C, int32_t S_d, int32_t F, int32_t chunks, float* __restrict__ g_rows) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t w = static_cast<int64_t>(blockIdx.x) * (kPgThreads / kWave) + (threadIdx.x >> 6);
    if (w >= static_cast<int64_t>(S_d) * chunks) return;                    // (whole waves leave: the ballots below see full waves)
    const int32_t j = static_cast<int32_t>(w / chunks), chunk = static_cast<int32_t>(w - static_cast<int64_t>(j) * chunks);
    const int32_t p0 = min(max(seq_pair[j], 0), B * C - 1);
    const int32_t b = p0 / C;
    const int32_t col = (chunk * kWave + lane) * VEC;
    const bool live = col < F;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    for (int32_t c0 = 0; c0 < C; c0 += kWave) {
        const int32_t c = c0 + lane;
        unsigned long long m = __ballot(c < C && pair_seq[b * C + min(c, C - 1)] == j);
        while (m) {
            const int bit = __ffsll(static_cast<long long>(m)) - 1;
            m &= m - 1;
            if (live) {
                float x[VEC];
                load_vec<VEC>(x, g_out + (static_cast<int64_t>(b) * C + c0 + bit) * F + col);
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] += x[e];
            }
        }
    }
    if (live) store_vec<VEC>(g_rows + static_cast<int64_t>(j) * F + col, acc);
}

bool pg_shape_ok(int64_t B, int64_t C, int64_t T) {
    return B >= 1 && B <= kPgMaxB && C >= 1 && C <= kPgMaxC && T >= 1 && B * C * T < kPgMaxCells;
}

constexpr size_t kPgLocalLds = 48 * 1024;             // a sentence's rows staged in LDS up to this size; read in place (L1 / L2) above

template <typename WT>
void pg_launch_local(hipStream_t st, const void* markers, int64_t row_bytes, int32_t B, int32_t C, int32_t* first, int32_t* lrank, int32_t* counts) {
    const int32_t words = static_cast<int32_t>(row_bytes / static_cast<int64_t>(sizeof(WT)));
    const size_t lds = static_cast<size_t>(C) * static_cast<size_t>(row_bytes);
    if (lds <= kPgLocalLds)
        hipLaunchKernelGGL((k_pg_local<WT, true>), dim3(static_cast<unsigned>(B)), dim3(kPgMaxC), lds, st, static_cast<const WT*>(markers), words, C, first, lrank,
                           counts);
    else
        hipLaunchKernelGGL((k_pg_local<WT, false>), dim3(static_cast<unsigned>(B)), dim3(kPgMaxC), 0, st, static_cast<const WT*>(markers), words, C, first, lrank,
                           counts);
}

template <typename ST, typename MT, typename OT>
void pg_launch_scan(hipStream_t st, const void* sentence, const void* markers, const int32_t* first, const int32_t* lrank, const int32_t* counts, int32_t B,
                    int32_t C, int32_t T, int32_t total, int32_t* seq_pair, int32_t* pair_seq, int32_t* seq_ptr, void* sentence_d, void* markers_d,
                    int32_t* status) {
    hipLaunchKernelGGL((k_pg_scan<ST, MT, OT>), dim3(1), dim3(kPgScanThreads), 0, st, static_cast<const ST*>(sentence), static_cast<const MT*>(markers), first,
                       lrank, counts, B, C, T, total, seq_pair, pair_seq, seq_ptr, static_cast<OT*>(sentence_d), static_cast<OT*>(markers_d), status);
}

template <typename ST>
void pg_scan_markers(hipStream_t st, int32_t marker_bytes, const void* sentence, const void* markers, const int32_t* first, const int32_t* lrank,
                     const int32_t* counts, int32_t B, int32_t C, int32_t T, int32_t total, int32_t* seq_pair, int32_t* pair_seq, int32_t* seq_ptr,
                     void* sentence_d, void* markers_d, int32_t* status) {
    if (marker_bytes == 1)
        pg_launch_scan<ST, int8_t, ST>(st, sentence, markers, first, lrank, counts, B, C, T, total, seq_pair, pair_seq, seq_ptr, sentence_d, markers_d, status);
    else if (marker_bytes == 4)
        pg_launch_scan<ST, int32_t, ST>(st, sentence, markers, first, lrank, counts, B, C, T, total, seq_pair, pair_seq, seq_ptr, sentence_d, markers_d, status);
    else
        pg_launch_scan<ST, int64_t, ST>(st, sentence, markers, first, lrank, counts, B, C, T, total, seq_pair, pair_seq, seq_ptr, sentence_d, markers_d, status);
}

bool pg_vec4(const void* a, const void* b, int32_t F) {
    return F % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0;
}

}  // namespace
}  // namespace recon

extern "C" int recon_pair_groups_supported(int64_t B, int64_t C, int64_t T) { return recon::pg_shape_ok(B, C, T) ? 1 : 0; }

extern "C" size_t recon_pair_groups_workspace_bytes(int64_t B, int64_t C, int64_t T) {
    if (!recon::pg_shape_ok(B, C, T)) return 0;
    return align_up(static_cast<size_t>(2 * B * C + B) * sizeof(int32_t), 16);
}

extern "C" int recon_pair_groups_local(const void* markers, int32_t marker_bytes, int64_t B, int64_t C, int64_t T, int32_t* first, int32_t* local_rank,
                                       int32_t* counts, recon_stream_t stream) {
    using namespace recon;
    if (B < 1 || C < 1 || T < 1 || (marker_bytes != 1 && marker_bytes != 4 && marker_bytes != 8)) return RECON_ERR_INVALID;
    if (!markers || !first || !local_rank || !counts) return RECON_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(markers) % static_cast<uintptr_t>(marker_bytes)) return RECON_ERR_INVALID;
    if (!pg_shape_ok(B, C, T)) return RECON_ERR_UNSUPPORTED;
    const int64_t row_bytes = T * marker_bytes;
    const uintptr_t a = reinterpret_cast<uintptr_t>(markers) | static_cast<uintptr_t>(row_bytes);
    const hipStream_t st = as_stream(stream);
    const int32_t b = static_cast<int32_t>(B), c = static_cast<int32_t>(C);
    if (a % 8 == 0) pg_launch_local<uint64_t>(st, markers, row_bytes, b, c, first, local_rank, counts);
    else if (a % 4 == 0) pg_launch_local<uint32_t>(st, markers, row_bytes, b, c, first, local_rank, counts);
    else if (a % 2 == 0) pg_launch_local<uint16_t>(st, markers, row_bytes, b, c, first, local_rank, counts);
    else pg_launch_local<uint8_t>(st, markers, row_bytes, b, c, first, local_rank, counts);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_pair_groups_build(const void* sentence, int32_t index_bytes, const void* markers, int32_t marker_bytes, int64_t B, int64_t C, int64_t T,
                                       int64_t total, int32_t* seq_pair, int32_t* pair_seq, int32_t* seq_ptr, void* sentence_d, void* markers_d,
                                       int32_t* status, void* workspace, size_t workspace_bytes, recon_stream_t stream) {
    using namespace recon;
    if (B < 1 || C < 1 || T < 1 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (!pair_seq || !seq_ptr || !workspace) return RECON_ERR_INVALID;
    if (total >= 0 && (!sentence || !seq_pair || !sentence_d || !markers_d || !status || total < B || total > B * C)) return RECON_ERR_INVALID;
    if (total >= 0 && ((reinterpret_cast<uintptr_t>(sentence) | reinterpret_cast<uintptr_t>(sentence_d) | reinterpret_cast<uintptr_t>(markers_d)) %
                       static_cast<uintptr_t>(index_bytes)))
        return RECON_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return RECON_ERR_INVALID;
    if (!pg_shape_ok(B, C, T)) return RECON_ERR_UNSUPPORTED;
    if (workspace_bytes < recon_pair_groups_workspace_bytes(B, C, T)) return RECON_ERR_WORKSPACE;
    int32_t* first = static_cast<int32_t*>(workspace);
    int32_t* lrank = first + B * C;
    int32_t* counts = lrank + B * C;
    const int rc = recon_pair_groups_local(markers, marker_bytes, B, C, T, first, lrank, counts, stream);
    if (rc != RECON_OK) return rc;
    const hipStream_t st = as_stream(stream);
    const int32_t b = static_cast<int32_t>(B), c = static_cast<int32_t>(C), t = static_cast<int32_t>(T), tot = total < 0 ? -1 : static_cast<int32_t>(total);
    if (index_bytes == 8)
        pg_scan_markers<int64_t>(st, marker_bytes, sentence, markers, first, lrank, counts, b, c, t, tot, seq_pair, pair_seq, seq_ptr, sentence_d, markers_d, status);
    else
        pg_scan_markers<int32_t>(st, marker_bytes, sentence, markers, first, lrank, counts, b, c, t, tot, seq_pair, pair_seq, seq_ptr, sentence_d, markers_d, status);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_pair_groups_expand(const float* rows, const int32_t* pair_seq, int64_t n_pairs, int64_t S_d, int32_t F, float* out, recon_stream_t stream) {
    using namespace recon;
    if (n_pairs < 0 || S_d < 0 || F < 1 || (n_pairs > 0 && (S_d < 1 || !rows || !pair_seq || !out))) return RECON_ERR_INVALID;
    if (n_pairs * F >= kPgMaxCells || S_d * F >= kPgMaxCells) return RECON_ERR_UNSUPPORTED;
    if (n_pairs == 0) return RECON_OK;
    const int32_t n = static_cast<int32_t>(n_pairs), s = static_cast<int32_t>(S_d);
    if (pg_vec4(rows, out, F))
        hipLaunchKernelGGL((k_pg_expand<4>), dim3(static_cast<unsigned>(ceil_div64(n_pairs * (F / 4), kPgThreads))), dim3(kPgThreads), 0, as_stream(stream), rows,
                           pair_seq, n, s, F, out);
    else
        hipLaunchKernelGGL((k_pg_expand<1>), dim3(static_cast<unsigned>(ceil_div64(n_pairs * F, kPgThreads))), dim3(kPgThreads), 0, as_stream(stream), rows,
                           pair_seq, n, s, F, out);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_pair_groups_reduce(const float* g_out, const int32_t* pair_seq, const int32_t* seq_pair, int64_t B, int64_t C, int64_t S_d, int32_t F,
                                        float* g_rows, recon_stream_t stream) {
    using namespace recon;
    if (B < 0 || C < 1 || S_d < 0 || F < 1 || (B > 0 && (!g_out || !pair_seq)) || (S_d > 0 && (B < 1 || !seq_pair || !g_rows))) return RECON_ERR_INVALID;
    if (B * C * F >= kPgMaxCells || S_d * F >= kPgMaxCells) return RECON_ERR_UNSUPPORTED;
    if (S_d == 0) return RECON_OK;
    const int32_t b = static_cast<int32_t>(B), c = static_cast<int32_t>(C), s = static_cast<int32_t>(S_d);
    constexpr int kWaves = kPgThreads / kWave;
    if (pg_vec4(g_out, g_rows, F)) {
        const int32_t chunks = (F / 4 + kWave - 1) / kWave;
        hipLaunchKernelGGL((k_pg_reduce<4>), dim3(static_cast<unsigned>(ceil_div64(S_d * chunks, kWaves))), dim3(kPgThreads), 0, as_stream(stream), g_out, pair_seq,
                           seq_pair, b, c, s, F, chunks, g_rows);
    } else {
        const int32_t chunks = (F + kWave - 1) / kWave;
        hipLaunchKernelGGL((k_pg_reduce<1>), dim3(static_cast<unsigned>(ceil_div64(S_d * chunks, kWaves))), dim3(kPgThreads), 0, as_stream(stream), g_out, pair_seq,
                           seq_pair, b, c, s, F, chunks, g_rows);
    }
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}
