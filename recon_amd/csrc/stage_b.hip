// E15 — a stage-B iteration's two ends over a device-resident dataset (recon_amd/stage_b.py):
//   recon_stage_b_slice    train.py:247-251 with the casts of :261-262 and :309 (again :333-337, and test.py): the batch's rows of the
//                          dataset's compact arrays, widened to the dtypes the model and the objective take;
//   recon_stage_b_collect  test.py:285-292 and the indices of :300-302: the rows whose label is not ignored, in row order, appended behind
//                          what earlier batches of the pass left.
//   recon_pair_slice       the same cut for the per-pair baselines' datasets (recon_amd/pair_data.py; parsing/legacy_sp_models.py:67-97,
//                          :503-603, train.py:247-249, :301-309): one entity pair per row, and PCNN's segment mask unpacked from one byte per token.
// Selection and copying only: every output equals the reference's array to the value, `confidence` and the mask to the bit.
//
// k_sb_slice<kSegments, kPlanes>: ONE launch for all outputs (seven of a StageBSlice: <7, false>; five of a PairSlice: <5, true>).
//   Each output is a flat run of 16-byte vectors, one per thread, the way k_cb_fill (ctx_batch.hip) writes its arrays: a wave's store instruction covers 1 KiB of consecutive bytes whatever the row width, and a base that
//   is not 16-byte aligned shifts the vector grid, so that only an array's first and last vector fall back to element stores.  Every cell
//   is written exactly once (the host hands torch.empty).  The dataset's row of batch row b is order[start + b] (start + b without an
//   order) CLAMPED into [0, N): the host validates an order where it enters, and the clamp keeps whatever it reads from ever becoming an
//   address.  Sources are int8, int16 or int32 and are sign-extended to the output's 4 or 8 bytes.  Flat output indices are int32
//   (recon_stage_b_supported refuses an output of 2^31 - 4096 cells or more); a source offset is 64-bit, the dataset may be larger.  No atomics.
//   kPlanes adds one kind of segment, a bit-plane source with a float32 destination: the dataset row is `width / 3` bytes, and output cell
//   j of a batch row is bit j / T of byte j % T as 0.0f or 1.0f (T = width / 3): the [3][T] mask of PCNN from one byte per token.
// k_sb_collect: ONE workgroup of 1024 threads walks the M rows in chunks of 1024, in order.  Within a chunk a ballot gives a kept row its
//   rank in its wave, a scan over the 16 wave counts its rank in the chunk: the compaction is stable.  The cursor is an int64 in the
//   caller's device state, read at the start and stored once at the end with plain loads and stores — launches on one stream are ordered,
//   so nothing here is atomic.  A row whose place is at or beyond the capacity is not stored; the cursor goes on counting and the state's
//   overflow word is set.
#include "recon_common.h"

namespace recon {
namespace {

constexpr int kSbThreads = 256;
constexpr int kSbCollectThreads = 1024;
constexpr int kSbSegments = 7;
constexpr int kPsSegments = 5;
constexpr int64_t kSbMaxCells = (int64_t{1} << 31) - 4096;      // of the largest output: a last vector's past-the-end indices still fit an int32

enum { SB_SRC_I8 = 1, SB_SRC_I16 = 2, SB_SRC_I32 = 4, SB_SRC_ROW = 0 };      // bytes of a source element; 0: the value is the dataset row itself
enum { SB_SRC_PLANES = 3 };                                                  // k_sb_slice<., true> only: uint8 [N][width / 3], three bit planes

struct SbSegment {
    void* dst;              // nullptr: the dataset has no such array
    const void* src;
    int32_t width;          // cells per dataset row
    int32_t total;          // count * width
    int32_t shift;          // cells from the last 16-byte boundary to dst
    int32_t dst_bytes;      // 4 or 8
    int32_t src_kind;
    int32_t block_end;      // first block behind this segment's
};
template <int kSegments>
struct SbSliceT {
    SbSegment seg[kSegments];
    const int64_t* order;   // nullptr: the identity
    int64_t start, N;
};
typedef SbSliceT<kSbSegments> SbSlice;
typedef SbSliceT<kPsSegments> PsSlice;

template <typename S>
__device__ __forceinline__ int64_t sb_row(const S& s, int32_t b) {
    const int64_t r = s.order ? s.order[s.start + b] : s.start + b;
    return r < 0 ? 0 : (r >= s.N ? s.N - 1 : r);
}

__device__ __forceinline__ int64_t sb_load(const SbSegment& g, int64_t row, int32_t j) {
    const int64_t at = row * g.width + j;
    switch (g.src_kind) {
        case SB_SRC_I8: return static_cast<const int8_t*>(g.src)[at];
        case SB_SRC_I16: return static_cast<const int16_t*>(g.src)[at];
        case SB_SRC_I32: return static_cast<const int32_t*>(g.src)[at];
        default: return row;
    }
}

// vector v of the segment's flat output: cells [v VE - shift, v VE - shift + VE); kPlanes: the segment is SB_SRC_PLANES
template <typename OT, bool kPlanes, typename S>
__device__ __forceinline__ void sb_slice_vec(const S& s, const SbSegment& g, int32_t v) {
    constexpr int VE = 16 / sizeof(OT);
    typedef OT vec_t __attribute__((ext_vector_type(VE)));
    OT* __restrict__ out = static_cast<OT*>(g.dst);
    const int64_t f0w = static_cast<int64_t>(v) * VE - g.shift;
    if (f0w >= g.total) return;                                       // (f0w + VE > 0 always: shift < VE)
    const int32_t f0 = static_cast<int32_t>(f0w);
    const int32_t fa = f0 < 0 ? 0 : f0;
    int32_t b = fa / g.width;
    int32_t j = fa - b * g.width;
    int64_t row = sb_row(s, b);
    const int32_t T = kPlanes ? g.width / 3 : 1;                      // planes: bytes per dataset row,
    int32_t p = kPlanes ? j / T : 0;                                  // the plane of cell j
    int32_t t = kPlanes ? j - p * T : 0;                              // and its token
    OT val[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        const int32_t f = f0 + e;
        val[e] = 0;
        if (f < 0 || f >= g.total) continue;
        if (kPlanes) {
            val[e] = static_cast<OT>((static_cast<const uint8_t*>(g.src)[row * T + t] >> p) & 1);
            if (++t == T) {
                t = 0;
                ++p;
            }
        } else {
            val[e] = static_cast<OT>(sb_load(g, row, j));
        }
        if (++j == g.width) {
            j = 0;
            p = 0;
            ++b;
            if (f + 1 < g.total && e + 1 < VE) row = sb_row(s, b);
        }
    }
    if (f0 >= 0 && f0 + VE <= g.total) {
        vec_t x;
#pragma unroll
        for (int e = 0; e < VE; ++e) x[e] = val[e];
        *reinterpret_cast<vec_t*>(out + f0) = x;
    } else {
#pragma unroll
        for (int e = 0; e < VE; ++e)
            if (f0 + e >= 0 && f0 + e < g.total) out[f0 + e] = val[e];
    }
}

template <int kSegments, bool kPlanes>
__global__ void __launch_bounds__(kSbThreads) k_sb_slice(const SbSliceT<kSegments> s) {
    const int32_t blk = static_cast<int32_t>(blockIdx.x);
    int32_t first = 0;
#pragma unroll
    for (int i = 0; i < kSegments; ++i) {
        const SbSegment& g = s.seg[i];
        if (blk < g.block_end) {
            const int32_t v = (blk - first) * kSbThreads + static_cast<int32_t>(threadIdx.x);
            if (kPlanes && g.src_kind == SB_SRC_PLANES) sb_slice_vec<float, true>(s, g, v);
            else if (g.dst_bytes == 8) sb_slice_vec<int64_t, false>(s, g, v);
            else sb_slice_vec<int32_t, false>(s, g, v);
            return;
        }
        first = g.block_end;
    }
}

__global__ void __launch_bounds__(kSbCollectThreads) k_sb_collect(const int64_t* __restrict__ labels, const int64_t* __restrict__ predicted,
                                                                   const float* __restrict__ confidence, const int64_t* __restrict__ rows, int64_t M,
                                                                   int64_t C, int64_t ignore_index, int64_t* __restrict__ state, int64_t capacity,
                                                                   int64_t* __restrict__ out_pair, int64_t* __restrict__ out_predicted,
                                                                   int64_t* __restrict__ out_gold, float* __restrict__ out_confidence) {
    constexpr int kWaves = kSbCollectThreads / kWave;
    __shared__ int32_t wave_count[2][kWaves];                        // two sets: a chunk's counts are still read while the next chunk's are written
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int64_t base = state[0];
    int64_t taken = 0;                                                // kept rows of the chunks in front of this one
    int set = 0;
    for (int64_t m0 = 0; m0 < M; m0 += kSbCollectThreads, set ^= 1) {
        const int64_t m = m0 + tid;
        int64_t gold = 0;
        bool keep = false;
        if (m < M) {
            gold = labels[m];
            keep = gold != ignore_index;
        }
        const unsigned long long votes = __ballot(keep);
        if (lane == 0) wave_count[set][wave] = __popcll(votes);
        __syncthreads();
        int32_t in_front = 0, chunk = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int32_t c = wave_count[set][w];
            in_front += w < wave ? c : 0;
            chunk += c;
        }
        if (keep) {
            const int64_t at = base + taken + in_front + __popcll(votes & ((1ull << lane) - 1ull));
            if (at < capacity) {
                out_pair[at] = rows[m / C] * C + m % C;
                out_predicted[at] = predicted[m];
                out_gold[at] = gold;
                out_confidence[at] = confidence[m];
            }
        }
        taken += chunk;
    }
    if (tid == 0) {
        state[0] = base + taken;
        if (base + taken > capacity) state[1] = 1;
    }
}

bool sb_shape_ok(int64_t count, int64_t C, int64_t T) {
    if (count < 1 || C < 1 || T < 1 || C >= kSbMaxCells || T >= kSbMaxCells || count >= kSbMaxCells || C * T >= kSbMaxCells) return false;
    return count * (C * (T > 2 ? T : 2)) < kSbMaxCells;              // the widest rows: markers C T, the id pairs 2 C
}

bool ps_shape_ok(int64_t count, int64_t marker_rows, int64_t T) {
    if (count < 1 || (marker_rows != 1 && marker_rows != 2) || T < 1 || T >= kSbMaxCells / 3 || count >= kSbMaxCells) return false;
    return count * (3 * T) < kSbMaxCells;                            // the widest rows: the mask's 3 T
}

// one output of the slice; returns the segment's blocks
int32_t sb_segment(SbSegment* g, void* dst, const void* src, int64_t width, int64_t count, int32_t dst_bytes, int32_t src_kind, int32_t first_block) {
    g->dst = dst;
    g->src = src;
    g->width = static_cast<int32_t>(width);
    g->total = dst ? static_cast<int32_t>(count * width) : 0;
    g->shift = static_cast<int32_t>((reinterpret_cast<uintptr_t>(dst) & 15u) / static_cast<uintptr_t>(dst_bytes));
    g->dst_bytes = dst_bytes;
    g->src_kind = src_kind;
    const int64_t vectors = dst ? ceil_div64(static_cast<int64_t>(g->total) + g->shift, 16 / dst_bytes) : 0;
    const int32_t blocks = static_cast<int32_t>(ceil_div64(vectors, kSbThreads));
    g->block_end = first_block + blocks;
    return blocks;
}

}  // namespace
}  // namespace recon

extern "C" int recon_stage_b_supported(int64_t count, int64_t num_pairs, int64_t sent_len) {
    return recon::sb_shape_ok(count, num_pairs, sent_len) ? 1 : 0;
}

extern "C" int recon_stage_b_slice(const int32_t* sentences, const int8_t* markers, const int16_t* labels, const int32_t* num_entities,
                                   const int32_t* entity_indices, const int32_t* surface_ids, int64_t N, int64_t num_pairs, int64_t sent_len,
                                   const int64_t* order, int64_t order_len, int64_t start, int64_t count, int32_t index_bytes,
                                   void* sentence_input, void* entity_markers, int64_t* labels_out, int32_t* num_entities_out,
                                   int64_t* entity_indices_out, int32_t* surface_ids_out, int64_t* rows_out, recon_stream_t stream) {
    using namespace recon;
    if (!sentences || !markers || !labels || !num_entities || !sentence_input || !entity_markers || !labels_out || !num_entities_out || !rows_out)
        return RECON_ERR_INVALID;
    if ((entity_indices == nullptr) != (entity_indices_out == nullptr) || (surface_ids == nullptr) != (surface_ids_out == nullptr)) return RECON_ERR_INVALID;
    if (N < 1 || num_pairs < 1 || sent_len < 1 || count < 1 || start < 0 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (order ? (order_len < 0 || start > order_len || count > order_len - start) : (start > N || count > N - start)) return RECON_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(sentence_input) | reinterpret_cast<uintptr_t>(entity_markers)) % static_cast<uintptr_t>(index_bytes))
        return RECON_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(labels_out) | reinterpret_cast<uintptr_t>(entity_indices_out) | reinterpret_cast<uintptr_t>(rows_out)) % 8u ||
        (reinterpret_cast<uintptr_t>(num_entities_out) | reinterpret_cast<uintptr_t>(surface_ids_out)) % 4u)
        return RECON_ERR_INVALID;
    if (!sb_shape_ok(count, num_pairs, sent_len)) return RECON_ERR_UNSUPPORTED;
    SbSlice s;
    s.order = order;
    s.start = start;
    s.N = N;
    int32_t blocks = 0;
    blocks += sb_segment(&s.seg[0], entity_markers, markers, num_pairs * sent_len, count, index_bytes, SB_SRC_I8, blocks);
    blocks += sb_segment(&s.seg[1], sentence_input, sentences, sent_len, count, index_bytes, SB_SRC_I32, blocks);
    blocks += sb_segment(&s.seg[2], labels_out, labels, num_pairs, count, 8, SB_SRC_I16, blocks);
    blocks += sb_segment(&s.seg[3], entity_indices_out, entity_indices, 2 * num_pairs, count, 8, SB_SRC_I32, blocks);
    blocks += sb_segment(&s.seg[4], surface_ids_out, surface_ids, 2 * num_pairs, count, 4, SB_SRC_I32, blocks);
    blocks += sb_segment(&s.seg[5], num_entities_out, num_entities, 1, count, 4, SB_SRC_I32, blocks);
    blocks += sb_segment(&s.seg[6], rows_out, nullptr, 1, count, 8, SB_SRC_ROW, blocks);
    hipLaunchKernelGGL((k_sb_slice<kSbSegments, false>), dim3(static_cast<unsigned>(blocks)), dim3(kSbThreads), 0, as_stream(stream), s);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_pair_slice_supported(int64_t count, int64_t marker_rows, int64_t sent_len) {
    return recon::ps_shape_ok(count, marker_rows, sent_len) ? 1 : 0;
}

extern "C" int recon_pair_slice(const int32_t* sentences, const int8_t* markers, const int16_t* labels, const uint8_t* segment_bits, int64_t N,
                                int64_t marker_rows, int64_t sent_len, const int64_t* order, int64_t order_len, int64_t start, int64_t count,
                                int32_t index_bytes, void* sentence_input, void* entity_markers, float* pcnn_mask, int64_t* labels_out,
                                int64_t* rows_out, recon_stream_t stream) {
    using namespace recon;
    if (!sentences || !markers || !labels || !sentence_input || !entity_markers || !labels_out || !rows_out) return RECON_ERR_INVALID;
    if ((segment_bits == nullptr) != (pcnn_mask == nullptr)) return RECON_ERR_INVALID;
    if (N < 1 || (marker_rows != 1 && marker_rows != 2) || sent_len < 1 || count < 1 || start < 0 || (index_bytes != 4 && index_bytes != 8))
        return RECON_ERR_INVALID;
    if (order ? (order_len < 0 || start > order_len || count > order_len - start) : (start > N || count > N - start)) return RECON_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(sentence_input) | reinterpret_cast<uintptr_t>(entity_markers)) % static_cast<uintptr_t>(index_bytes))
        return RECON_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(labels_out) | reinterpret_cast<uintptr_t>(rows_out)) % 8u || reinterpret_cast<uintptr_t>(pcnn_mask) % 4u)
        return RECON_ERR_INVALID;
    if (!ps_shape_ok(count, marker_rows, sent_len)) return RECON_ERR_UNSUPPORTED;
    PsSlice s;
    s.order = order;
    s.start = start;
    s.N = N;
    int32_t blocks = 0;
    blocks += sb_segment(&s.seg[0], pcnn_mask, segment_bits, 3 * sent_len, count, 4, SB_SRC_PLANES, blocks);
    blocks += sb_segment(&s.seg[1], entity_markers, markers, marker_rows * sent_len, count, index_bytes, SB_SRC_I8, blocks);
    blocks += sb_segment(&s.seg[2], sentence_input, sentences, sent_len, count, index_bytes, SB_SRC_I32, blocks);
    blocks += sb_segment(&s.seg[3], labels_out, labels, 1, count, 8, SB_SRC_I16, blocks);
    blocks += sb_segment(&s.seg[4], rows_out, nullptr, 1, count, 8, SB_SRC_ROW, blocks);
    hipLaunchKernelGGL((k_sb_slice<kPsSegments, true>), dim3(static_cast<unsigned>(blocks)), dim3(kSbThreads), 0, as_stream(stream), s);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_stage_b_collect(const int64_t* labels, const int64_t* predicted, const float* confidence, const int64_t* rows, int64_t M,
                                     int64_t num_pairs, int64_t ignore_index, int64_t* state, int64_t capacity, int64_t* out_pair,
                                     int64_t* out_predicted, int64_t* out_gold, float* out_confidence, recon_stream_t stream) {
    using namespace recon;
    if (!labels || !predicted || !confidence || !rows || !state) return RECON_ERR_INVALID;
    if (M < 1 || num_pairs < 1 || M % num_pairs != 0 || capacity < 0) return RECON_ERR_INVALID;
    if (capacity > 0 && (!out_pair || !out_predicted || !out_gold || !out_confidence)) return RECON_ERR_INVALID;
    hipLaunchKernelGGL(k_sb_collect, dim3(1), dim3(kSbCollectThreads), 0, as_stream(stream), labels, predicted, confidence, rows, M, num_pairs,
                       ignore_index, state, capacity, out_pair, out_predicted, out_gold, out_confidence);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}
