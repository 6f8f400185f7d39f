// E14 — the stage-B entity-context batch between the dataset's index arrays and the model's inputs (train.py:250-258, :337-344, test.py):
// utils/context_utils.py:62-84 get_batch_unique_entities, :293-301 get_entity_location_unique_entities, :365-385 get_context_indices
// (with :120-152, :256-291, :303-319 behind it) and :444-475 get_gat_entity_embeddings / get_selected_gat_entity_embeddings, over
// tables that recon_amd/context_batch.py builds once per dataset.  Selection, ordering and copying only: every output equals the
// reference's array to the value (floats to the bit).  No atomics on global memory; every LDS atomic is an integer min / max / add / or,
// whose result does not depend on the order of arrival, so the outputs are the same bits from run to run.
//
// k_cb_index: ONE workgroup of 1024 threads over the n = 2 B C ids of the batch.
//   1. every id goes into an open-addressing hash table in LDS (key = id + 1, linear probing, ds_cmpst to claim a slot) that keeps the
//      id's lowest position (ds_min), highest position (ds_max) and count (ds_add).  H = the power of two >= 2 n, at most 8192 slots of
//      16 bytes = 128 KiB of the 160 KiB of LDS; n <= 8192 ids always fit (the table may then be full: a probe sequence still ends,
//      there are at most n distinct keys).  The reference's batch is 7200 ids.
//   2. every id other than -1 sets the bit of its lowest position in a bitmap of n bits; a scan of the bitmap's word counts (one wave,
//      four words per lane, __shfl_up) turns a position into the number of first occurrences in front of it: the id's rank in dict
//      insertion order.  -1 has rank 0 whether it occurs or not (context_utils.py:63-64 seeds the dicts with it).
//   3. the slot's owner writes unique_entities[rank], the entity's line count and the surface id at its HIGHEST position (:68 overwrites:
//      the last occurrence wins), and feeds three LDS maxima: lines (P_b), tokens of the longest line (T_b) and (count << 16 | 0xffff -
//      rank), whose maximum is the FIRST maximum of the counts in rank order (np.argmax, :80).
//   4. every position looks its id up again and writes its rank (entities_position).
//   5. the pairs with a half other than -1 set a bit each; the same scan gives nonzero_entity_pos and every pair's row in the compacted
//      block (:471-474).
//   An id outside [-1, Ne) or a surface id outside [0, S) sets a flag in the header and is never used as an address.
// k_cb_fill: the three context arrays as flat runs of 16-byte vectors — a wave's store instruction covers 1 KiB of consecutive bytes —
//   whatever the row width; a base that is not 16-byte aligned shifts the vector grid, so that only the first and last vector of an
//   array fall back to element stores.  Every cell is written exactly once (the host hands torch.empty).
// k_cb_scan + k_cb_fill over CbRaggedRows (recon_ctx_batch_fill_ragged): the same two arrays without the padding lines, [L][T_b] and [L][W] with
//   L = header[6] = the sum of the entities' line counts, which k_cb_index adds up in LDS (an integer add: any order, one result).  One workgroup
//   scans the counts in rank order into line_ptr [U + 1] and writes the owner of every row into row_ent [L]; the fill's vectors then find
//   (entity, line) of a row by two loads, row_ent[row] and line_ptr[u], where a search of line_ptr would be 13 dependent loads for the 8193
//   entities a batch can hold.  The map is L int32, at most 1/386 of the char block at the reference's widths.  No mask is written: every row is present.
// k_cb_forms_mark, k_cb_forms_scan, k_cb_forms_fill (recon_ctx_batch_forms_count, recon_ctx_batch_fill_forms): the char block
//   as its distinct word windows.  The tables carry a form id per token (tok_form; form 0 = the empty slot's all-pad row) and the forms' char
//   rows (form_chars).  Behind k_cb_index and in front of the host's read, k_cb_forms_mark walks the batch's lines by the sizes the header holds ON THE
//   DEVICE and stores 1 into flags[form] for every token's form, and into flags[0] where a line ends in front of T_b (same-value stores: any
//   order, one result); ONE workgroup then scans the flags in tiles of 4096 into rank[form] = the present forms below it, lists the present
//   forms and writes their number S_d into the header's eighth word.  After the read k_cb_forms_fill writes slot_form [rows T_b] = rank[form of the
//   slot's token] and chars [S_d][cfs - 1 + mcl + cfs - 1]; the dense [rows][W] block is never written.
// k_cb_gat: a wave per (b, c) pair writes both halves of gat_entity_embeddings and, for a present pair, the row of the compacted block.
#include "recon_common.h"

namespace recon {
namespace {

constexpr int kCbThreads = 1024;
constexpr int kCbMaxIds = 8192;                       // ids per batch: 16 bytes of table per id + 2 KiB of bitmap and scan, of 160 KiB
constexpr int kCbWords = kCbMaxIds / 32;              // bitmap words
static_assert(kCbWords == 4 * kWave, "cb_scan_words: one wave, four words per lane");
constexpr uint32_t kCbEmpty = 0xffffffffu;
constexpr int kCbFillThreads = 256;
constexpr int64_t kCbMaxCells = (int64_t{1} << 31) - 4096;      // of context_chars, the largest output

enum { CB_ERR_ID = 1, CB_ERR_SURFACE = 2, CB_ERR_HALF = 4, CB_ERR_MISSING = 8 };
enum { CB_T_LINE_PTR, CB_T_MAX_LEN, CB_T_LINE_START, CB_T_LINE_LEN, CB_T_SF_START, CB_T_SF_LEN, CB_T_FLAT, CB_T_WORD, CB_T_CHARS, CB_T_GAT_ROW,
       CB_T_GAT_EMB, CB_T_COUNT };
enum { CB_D_NE, CB_D_S, CB_D_V, CB_D_L, CB_D_NF, CB_D_MAX_T, CB_D_MAX_P, CB_D_MCL, CB_D_CFS, CB_D_PAD, CB_D_G, CB_D_NG, CB_D_COUNT };

struct CbTables {
    int64_t Ne, S;
    int32_t max_T, max_P, mcl, cfs, pad, G;
    const int32_t* ent_line_ptr;   // [Ne + 2]: table lines of id e are [ptr[e + 1], ptr[e + 2])
    const int32_t* ent_max_len;    // [Ne + 1]: tokens of the longest table line of id e, at e + 1; -1: no entity has this id
    const int32_t* line_start;     // [L] into tok_flat
    const int32_t* line_len;       // [L], cut at max_T
    const int32_t* sf_start;       // [S] into tok_flat
    const int32_t* sf_len;         // [S], cut at max_T
    const int32_t* tok_flat;
    const int32_t* tok_word;       // [V]
    const int32_t* tok_chars;      // [V][mcl], the pad char behind the token's end
    const int32_t* gat_row;        // [Ne + 1] at e + 1: row of gat_emb, -1: zeros, -2: missing
    const float* gat_emb;          // [Ng][G]
};

__device__ __forceinline__ uint32_t cb_slot0(uint32_t key, uint32_t H) { return ((key * 2654435761u) >> 12) & (H - 1); }

__device__ __forceinline__ uint32_t cb_find(const uint32_t* keys, uint32_t H, uint32_t key) {
    uint32_t h = cb_slot0(key, H);
    while (keys[h] != key) h = (h + 1) & (H - 1);
    return h;
}

// exclusive prefix sums of the popcounts of bits[0 .. kCbWords) into wpre, the total into *total; called by the 64 lanes of wave 0
__device__ __forceinline__ void cb_scan_words(const uint32_t* bits, uint32_t* wpre, uint32_t* total, int lane) {
    uint32_t c[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { c[j] = __popc(bits[4 * lane + j]); sum += c[j]; }
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    uint32_t run = incl - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) { wpre[4 * lane + j] = run; run += c[j]; }
    if (lane == 63) *total = incl;
}

__device__ __forceinline__ uint32_t cb_rank_of_bit(const uint32_t* bits, const uint32_t* wpre, uint32_t p) {
    return wpre[p >> 5] + __popc(bits[p >> 5] & ((1u << (p & 31)) - 1u));
}

__global__ void __launch_bounds__(kCbThreads) k_cb_index(const CbTables t, const int64_t* __restrict__ ids, const int32_t* __restrict__ surf, int32_t n,
                                                         uint32_t H, int32_t gat_mode, int64_t* __restrict__ uniq, int32_t* __restrict__ uinfo,
                                                         int64_t* __restrict__ pos, int64_t* __restrict__ nzpos, int32_t* __restrict__ pair_slot,
                                                         int32_t* __restrict__ hdr) {
    extern __shared__ __attribute__((aligned(16))) uint32_t cb_sm[];
    uint32_t* keys = cb_sm;
    uint32_t* minp = keys + H;
    uint32_t* maxp = minp + H;
    uint32_t* cnt = maxp + H;
    uint32_t* bits = cnt + H;
    uint32_t* wpre = bits + kCbWords;
    uint32_t* misc = wpre + kCbWords;          // 0 err, 1 -1 occurs, 2 longest line, 3 most lines, 4 count key, 5 first occurrences, 6 present pairs,
                                               // 7 the lines of all entities (each cut at max_P): the rows of the ragged form
    const int tid = threadIdx.x;
    for (uint32_t s = tid; s < H; s += kCbThreads) { keys[s] = kCbEmpty; minp[s] = 0xffffffffu; maxp[s] = 0; cnt[s] = 0; }
    if (tid < kCbWords) bits[tid] = 0;
    if (tid < 8) misc[tid] = tid == 4 ? 0xffffu : 0u;
    __syncthreads();
    // 1. the table
    for (int p = tid; p < n; p += kCbThreads) {
        const int64_t id = ids[p];
        const int32_t sid = surf[p];
        uint32_t err = 0;
        if (sid < 0 || sid >= t.S) err |= CB_ERR_SURFACE;
        if (id < -1 || id >= t.Ne) {
            err |= CB_ERR_ID;
        } else {
            const uint32_t key = static_cast<uint32_t>(id + 1);
            if (t.ent_max_len[key] < 0) err |= CB_ERR_ID;             // an id inside the range that no entity has
            uint32_t h = cb_slot0(key, H);
            for (;;) {
                const uint32_t old = atomicCAS(&keys[h], kCbEmpty, key);
                if (old == kCbEmpty || old == key) break;
                h = (h + 1) & (H - 1);
            }
            atomicMin(&minp[h], static_cast<uint32_t>(p));
            atomicMax(&maxp[h], static_cast<uint32_t>(p));
            atomicAdd(&cnt[h], 1u);
        }
        if (err) atomicOr(&misc[0], err);
    }
    __syncthreads();
    // 2. first occurrences -> ranks
    for (uint32_t s = tid; s < H; s += kCbThreads)
        if (keys[s] != kCbEmpty && keys[s] != 0u) atomicOr(&bits[minp[s] >> 5], 1u << (minp[s] & 31));
    __syncthreads();
    if (tid < 64) cb_scan_words(bits, wpre, &misc[5], tid);
    __syncthreads();
    // 3. one thread per distinct id
    for (uint32_t s = tid; s < H; s += kCbThreads) {
        const uint32_t key = keys[s];
        if (key == kCbEmpty) continue;
        const uint32_t r = key == 0u ? 0u : 1u + cb_rank_of_bit(bits, wpre, minp[s]);
        minp[s] = r;                                                  // the slot now answers "which rank"
        int32_t sid = surf[maxp[s]];
        if (sid < 0 || sid >= t.S) sid = 0;                           // flagged above; never an address
        const int32_t nl = 1 + t.ent_line_ptr[key + 1] - t.ent_line_ptr[key];
        uniq[r] = static_cast<int64_t>(key) - 1;
        uinfo[2 * r] = nl;
        uinfo[2 * r + 1] = sid;
        atomicMax(&misc[3], static_cast<uint32_t>(nl));
        atomicAdd(&misc[7], static_cast<uint32_t>(min(nl, t.max_P)));
        atomicMax(&misc[2], static_cast<uint32_t>(max(t.ent_max_len[key], t.sf_len[sid])));
        atomicMax(&misc[4], (cnt[s] << 16) | (0xffffu - r));
        if (key == 0u) misc[1] = 1u;
    }
    __syncthreads();
    if (tid == 0 && !misc[1]) {                                       // -1 does not occur: ['ALL_ZERO'] (surface 0), count 0
        const int32_t nl = 1 + t.ent_line_ptr[1] - t.ent_line_ptr[0];
        uniq[0] = -1;
        uinfo[0] = nl;
        uinfo[1] = 0;
        atomicMax(&misc[3], static_cast<uint32_t>(nl));
        atomicAdd(&misc[7], static_cast<uint32_t>(min(nl, t.max_P)));
        atomicMax(&misc[2], static_cast<uint32_t>(max(t.ent_max_len[0], t.sf_len[0])));
    }
    // 4. positions
    for (int p = tid; p < n; p += kCbThreads) {
        const int64_t id = ids[p];
        pos[p] = (id < -1 || id >= t.Ne) ? 0 : static_cast<int64_t>(minp[cb_find(keys, H, static_cast<uint32_t>(id + 1))]);
    }
    __syncthreads();
    // 5. pairs
    if (tid < kCbWords) bits[tid] = 0;
    __syncthreads();
    const int npairs = n >> 1;
    for (int q = tid; q < npairs; q += kCbThreads) {
        const int64_t a = ids[2 * q], b = ids[2 * q + 1];
        const bool va = a >= -1 && a < t.Ne, vb = b >= -1 && b < t.Ne;
        uint32_t err = 0;
        if (gat_mode && ((va && t.gat_row[a + 1] == -2) || (vb && t.gat_row[b + 1] == -2))) err |= CB_ERR_MISSING;
        if (gat_mode == 2 && va && vb) {
            if ((a != -1) != (b != -1)) err |= CB_ERR_HALF;
            if (a != -1 || b != -1) atomicOr(&bits[q >> 5], 1u << (q & 31));
        }
        if (err) atomicOr(&misc[0], err);
    }
    __syncthreads();
    if (tid < 64) cb_scan_words(bits, wpre, &misc[6], tid);
    __syncthreads();
    for (int q = tid; q < npairs; q += kCbThreads) {
        const bool present = (bits[q >> 5] >> (q & 31)) & 1u;
        const int32_t slot = present ? static_cast<int32_t>(cb_rank_of_bit(bits, wpre, static_cast<uint32_t>(q))) : -1;
        pair_slot[q] = slot;
        if (present) nzpos[slot] = q;
    }
    if (tid == 0) {
        hdr[0] = static_cast<int32_t>(1u + misc[5]);
        hdr[1] = min(t.max_T, static_cast<int32_t>(misc[2]));
        hdr[2] = min(t.max_P, static_cast<int32_t>(misc[3]));
        hdr[3] = static_cast<int32_t>(misc[6]);
        hdr[4] = static_cast<int32_t>(0xffffu - (misc[4] & 0xffffu));
        hdr[5] = static_cast<int32_t>(misc[0]);
        hdr[6] = static_cast<int32_t>(misc[7]);
        hdr[7] = 0;
    }
}

// tokens of line p of unique entity u: the surface form of its last occurrence, then the entity's table lines; nothing from its line count on
struct CbLine { int32_t start, len; };
// where row `row` of the context arrays lies: P rows per entity (the padded form), or the entity's own rows one after another (the ragged
// form: entity u owns the rows line_ptr[u] .. line_ptr[u + 1], and row_ent[row], written by k_cb_scan, names the owner of a row)
struct CbPaddedRows {
    static constexpr bool kMask = true;
    int32_t P;
    __device__ __forceinline__ void at(int32_t row, int32_t& u, int32_t& p) const { u = row / P; p = row - u * P; }
};
struct CbRaggedRows {
    static constexpr bool kMask = false;
    const int32_t* line_ptr;
    const int32_t* row_ent;
    __device__ __forceinline__ void at(int32_t row, int32_t& u, int32_t& p) const { u = row_ent[row]; p = row - line_ptr[u]; }
};
template <typename ROWS>
__device__ __forceinline__ CbLine cb_line(const CbTables& t, const int64_t* __restrict__ uniq, const int32_t* __restrict__ uinfo, int32_t row, const ROWS& rows, int32_t T) {
    int32_t u, p;
    rows.at(row, u, p);
    CbLine ln{0, 0};
    if (p == 0) {
        const int32_t sid = uinfo[2 * u + 1];
        ln.start = t.sf_start[sid];
        ln.len = t.sf_len[sid];
    } else if (p < uinfo[2 * u]) {
        const int32_t l = t.ent_line_ptr[uniq[u] + 1] + p - 1;
        ln.start = t.line_start[l];
        ln.len = t.line_len[l];
    }
    ln.len = min(ln.len, T);
    return ln;
}

// vector v of the flat array out[total] (rows of width W): elements [v VE - shift, v VE - shift + VE), shift = elements from the last
// 16-byte boundary to out.  Flat indices are int32 (recon_ctx_batch_fill refuses an array of 2^31 cells: a 64-bit division costs as much as the
// rest of a vector).  One division finds the vector's row and column, one more the word slot w and the char c of a char column; from there they count up.
template <typename IT, int VE, bool CHARS, typename ROWS>
__device__ __forceinline__ void cb_fill_vec(const CbTables& t, const int64_t* __restrict__ uniq, const int32_t* __restrict__ uinfo, const ROWS& P, int32_t T,
                                            int32_t W, IT* __restrict__ out, int32_t total, int32_t shift, int32_t v) {
    typedef IT vec_t __attribute__((ext_vector_type(VE)));
    const int32_t f0 = v * VE - shift;
    if (f0 >= total || f0 + VE <= 0) return;
    const int32_t fa = f0 < 0 ? 0 : f0;
    int32_t row = fa / W;
    int32_t j = fa - row * W;
    CbLine ln = cb_line(t, uniq, uinfo, row, P, T);
    const int32_t lead = CHARS ? t.cfs - 1 : 0, stride = CHARS ? t.mcl + t.cfs - 1 : 1;      // a char row: `lead` pad columns, then T slots of `stride`
    int32_t w = 0, c = 0;                                                                    // column j = lead + w stride + c; both 0 in front of that
    if (CHARS && j > lead) {
        w = (j - lead) / stride;
        c = (j - lead) - w * stride;
    }
    IT val[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        const int32_t f = f0 + e;
        val[e] = 0;
        if (f < 0 || f >= total) continue;
        if constexpr (CHARS)
            val[e] = static_cast<IT>((j >= lead && w < ln.len && c < t.mcl) ? t.tok_chars[static_cast<int64_t>(t.tok_flat[ln.start + w]) * t.mcl + c] : t.pad);
        else
            val[e] = static_cast<IT>(j < ln.len ? t.tok_word[t.tok_flat[ln.start + j]] : 0);
        if (++j == W) {
            j = w = c = 0;
            ++row;
            if (f + 1 < total && e + 1 < VE) ln = cb_line(t, uniq, uinfo, row, P, T);
        } else if (CHARS && j > lead && ++c == stride) {
            c = 0;
            ++w;
        }
    }
    if (f0 >= 0 && f0 + VE <= total) {
        vec_t x;
#pragma unroll
        for (int e = 0; e < VE; ++e) x[e] = val[e];
        *reinterpret_cast<vec_t*>(out + f0) = x;
    } else {
#pragma unroll
        for (int e = 0; e < VE; ++e)
            if (f0 + e >= 0 && f0 + e < total) out[f0 + e] = val[e];
    }
}

// `rows` rows of either form; the mask blocks (the padded form alone) follow the word blocks
template <typename IT, typename ROWS>
__global__ void __launch_bounds__(kCbFillThreads) k_cb_fill(const CbTables t, const int64_t* __restrict__ uniq, const int32_t* __restrict__ uinfo, int32_t rows,
                                                            const ROWS P, int32_t T, IT* __restrict__ words, IT* __restrict__ chars,
                                                            uint8_t* __restrict__ mask, int64_t char_blocks, int64_t word_blocks, int32_t char_shift,
                                                            int32_t word_shift) {
    constexpr int VE = 16 / sizeof(IT);
    const int64_t blk = blockIdx.x;
    if (blk < char_blocks) {
        const int32_t W = t.cfs - 1 + T * (t.mcl + t.cfs - 1);
        cb_fill_vec<IT, VE, true>(t, uniq, uinfo, P, T, W, chars, rows * W, char_shift, static_cast<int32_t>(blk * kCbFillThreads + threadIdx.x));
    } else if (blk < char_blocks + word_blocks) {
        cb_fill_vec<IT, VE, false>(t, uniq, uinfo, P, T, T, words, rows * T, word_shift, static_cast<int32_t>((blk - char_blocks) * kCbFillThreads + threadIdx.x));
    } else if constexpr (ROWS::kMask) {
        const int32_t i = static_cast<int32_t>((blk - char_blocks - word_blocks) * kCbFillThreads + threadIdx.x);
        if (i < rows) mask[i] = i % P.P >= uinfo[2 * (i / P.P)] ? 1 : 0;
    }
}

// line_ptr [U + 1] = the exclusive scan, in rank order, of the entities' line counts (each cut at P), and row_ent [L]: the entity of every
// row.  One workgroup: thread i takes the entities [i per, (i + 1) per), per = ceil(U / 1024) <= 9; a wave scans its lanes' sums by
// __shfl_up, thread 0 the 16 wave totals.  Nothing is written behind row L.
__global__ void __launch_bounds__(kCbThreads) k_cb_scan(const int32_t* __restrict__ uinfo, int32_t U, int32_t P, int32_t L, int32_t* __restrict__ line_ptr,
                                                        int32_t* __restrict__ row_ent) {
    __shared__ uint32_t wsum[kCbThreads / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int per = (U + kCbThreads - 1) / kCbThreads;
    const int u0 = min(U, tid * per), u1 = min(U, u0 + per);
    uint32_t sum = 0;
    for (int u = u0; u < u1; ++u) sum += static_cast<uint32_t>(min(max(uinfo[2 * u], 0), P));
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
        for (int w = 0; w < kCbThreads / kWave; ++w) { const uint32_t s = wsum[w]; wsum[w] = run; run += s; }
    }
    __syncthreads();
    int32_t base = static_cast<int32_t>(wsum[wv] + incl - sum);
    for (int u = u0; u < u1; ++u) {
        const int32_t nl = min(max(uinfo[2 * u], 0), P);
        line_ptr[u] = base;
        for (int32_t i = 0; i < nl; ++i)
            if (base + i < L) row_ent[base + i] = u;
        base += nl;
    }
    if (tid == kCbThreads - 1) line_ptr[U] = base;
}

__global__ void __launch_bounds__(kCbFillThreads) k_cb_gat(const CbTables t, const int64_t* __restrict__ ids, int64_t npairs, const int32_t* __restrict__ pair_slot,
                                                           float* __restrict__ out, float* __restrict__ nz) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t q = static_cast<int64_t>(blockIdx.x) * (kCbFillThreads / kWave) + (threadIdx.x >> 6);
    if (q >= npairs) return;
    const int32_t G = t.G;
    int32_t r[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int64_t id = ids[2 * q + k];
        r[k] = (id >= 0 && id < t.Ne) ? t.gat_row[id + 1] : -1;
    }
    const int32_t slot = nz ? pair_slot[q] : -1;
    for (int32_t j = lane; j < 2 * G; j += kWave) {
        const int32_t k = j >= G, c = j - k * G, row = k ? r[1] : r[0];
        const float v = row >= 0 ? t.gat_emb[static_cast<int64_t>(row) * G + c] : 0.f;
        out[q * 2 * G + j] = v;
        if (slot >= 0) nz[static_cast<int64_t>(slot) * 2 * G + j] = v;
    }
}

// ---- the char block as its distinct word windows
struct CbForms {
    const int32_t* tok_form;       // [V]: the form of every token, 1 .. NFm - 1 (0: a token whose char row is all pad)
    const int32_t* form_chars;     // [NFm][mcl]; row 0 is all pad
    int32_t NFm, V, NF;
};
constexpr int kCbFormTile = 4 * kCbThreads;           // flags per scan step

// the table form in word slot w of a line (0 behind the line's end), clamped into the tables whatever memory holds
__device__ __forceinline__ int32_t cb_slot_form(const CbTables& t, const CbForms& fm, const CbLine& ln, int32_t w) {
    if (w >= ln.len) return 0;
    const int32_t tok = min(max(t.tok_flat[min(max(ln.start + w, 0), fm.NF - 1)], 0), fm.V - 1);
    return min(max(fm.tok_form[tok], 0), fm.NFm - 1);
}

// One thread per (entity, line) of the padded grid, by the sizes k_cb_index left in the header (the host has not read them yet): the
// forms of the line's tokens, and form 0 where the line is shorter than T_b.  ragged: the lines at and behind an entity's count do not exist.
__global__ void __launch_bounds__(kCbFillThreads) k_cb_forms_mark(const CbTables t, const CbForms fm, const int64_t* __restrict__ uniq,
                                                                  const int32_t* __restrict__ uinfo, const int32_t* __restrict__ hdr, int32_t max_U,
                                                                  int32_t ragged, int32_t* __restrict__ flags) {
    const int32_t U = min(max(hdr[0], 0), max_U), T = min(max(hdr[1], 0), t.max_T), P = min(max(hdr[2], 0), t.max_P);
    const int64_t items = static_cast<int64_t>(U) * P;
    const CbPaddedRows rows{max(P, 1)};
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kCbFillThreads + threadIdx.x; i < items; i += static_cast<int64_t>(gridDim.x) * kCbFillThreads) {
        const int32_t row = static_cast<int32_t>(i);
        if (ragged && row % P >= uinfo[2 * (row / P)]) continue;
        const CbLine ln = cb_line(t, uniq, uinfo, row, rows, T);
        for (int32_t w = 0; w < ln.len; ++w) flags[cb_slot_form(t, fm, ln, w)] = 1;
        if (ln.len < T) flags[0] = 1;
    }
}

// rank[f] = the set flags below f, form_of[r] = the r-th present form, hdr[7] = their number.  ONE workgroup, tiles of 4096 flags: a
// thread's four, a wave's sums by __shfl_up, the 16 wave totals by every thread, the carry in a register.
__global__ void __launch_bounds__(kCbThreads) k_cb_forms_scan(const int32_t* __restrict__ flags, int32_t NFm, int32_t* __restrict__ rank,
                                                              int32_t* __restrict__ form_of, int32_t* __restrict__ hdr) {
    __shared__ uint32_t wsum[kCbThreads / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    uint32_t carry = 0;
    for (int32_t base = 0; base < NFm; base += kCbFormTile) {
        const int32_t i0 = base + 4 * tid;
        uint32_t c[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { c[j] = (i0 + j < NFm && flags[i0 + j] != 0) ? 1u : 0u; sum += c[j]; }
        uint32_t incl = sum;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off, kWave);
            if (lane >= off) incl += o;
        }
        if (lane == kWave - 1) wsum[wv] = incl;
        __syncthreads();
        uint32_t below = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kCbThreads / kWave; ++w) { const uint32_t s = wsum[w]; below += w < wv ? s : 0u; all += s; }
        uint32_t run = carry + below + incl - sum;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < NFm) {
                rank[i0 + j] = static_cast<int32_t>(run);
                if (c[j]) form_of[run] = i0 + j;
                run += c[j];
            }
        carry += all;
        __syncthreads();                                                  // wsum is written again in the next tile
    }
    if (tid == 0) hdr[7] = static_cast<int32_t>(carry);
}

// blocks [0, slot_blocks): slot_form[row T + w] = rank[the slot's form]; behind them chars [S_d][Wf]: the present forms' windows
template <typename IT, typename ROWS>
__global__ void __launch_bounds__(kCbFillThreads) k_cb_forms_fill(const CbTables t, const CbForms fm, const int64_t* __restrict__ uniq,
                                                                  const int32_t* __restrict__ uinfo, int32_t n_rows, const ROWS P, int32_t T, int32_t S_d,
                                                                  const int32_t* __restrict__ rank, const int32_t* __restrict__ form_of,
                                                                  int64_t slot_blocks, int32_t* __restrict__ slot_form, IT* __restrict__ chars) {
    const int64_t blk = blockIdx.x;
    if (blk < slot_blocks) {
        const int64_t i = blk * kCbFillThreads + threadIdx.x;
        if (i >= static_cast<int64_t>(n_rows) * T) return;
        const int32_t row = static_cast<int32_t>(i / T), w = static_cast<int32_t>(i - static_cast<int64_t>(row) * T);
        const CbLine ln = cb_line(t, uniq, uinfo, row, P, T);
        slot_form[i] = min(max(rank[cb_slot_form(t, fm, ln, w)], 0), S_d - 1);
    } else {
        const int32_t Wf = 2 * (t.cfs - 1) + t.mcl;
        const int64_t i = (blk - slot_blocks) * kCbFillThreads + threadIdx.x;
        if (i >= static_cast<int64_t>(S_d) * Wf) return;
        const int32_t r = static_cast<int32_t>(i / Wf), c = static_cast<int32_t>(i - static_cast<int64_t>(r) * Wf) - (t.cfs - 1);
        const int32_t f = min(max(form_of[r], 0), fm.NFm - 1);
        chars[i] = static_cast<IT>((c >= 0 && c < t.mcl) ? fm.form_chars[static_cast<int64_t>(f) * t.mcl + c] : t.pad);
    }
}

bool cb_forms(const int64_t* dims, const int32_t* tok_form, const int32_t* form_chars, int64_t NFm, CbForms* fm) {
    if (!dims || !tok_form || !form_chars || NFm < 1 || NFm >= (int64_t{1} << 31) - kCbFormTile) return false;
    if (dims[CB_D_V] < 1 || dims[CB_D_V] >= (int64_t{1} << 31) || dims[CB_D_NF] < 1 || dims[CB_D_NF] >= (int64_t{1} << 31)) return false;
    fm->tok_form = tok_form;
    fm->form_chars = form_chars;
    fm->NFm = static_cast<int32_t>(NFm);
    fm->V = static_cast<int32_t>(dims[CB_D_V]);
    fm->NF = static_cast<int32_t>(dims[CB_D_NF]);
    return true;
}

template <typename IT, typename ROWS>
void cb_launch_forms_fill(hipStream_t st, const CbTables& t, const CbForms& fm, const int64_t* uniq, const int32_t* uinfo, int64_t n_rows, const ROWS& rows,
                          int32_t T, int32_t S_d, const int32_t* rank, const int32_t* form_of, int32_t* slot_form, void* chars) {
    const int64_t sb = ceil_div64(n_rows * T, kCbFillThreads);
    const int64_t cb = ceil_div64(static_cast<int64_t>(S_d) * (2 * (t.cfs - 1) + t.mcl), kCbFillThreads);
    if (sb + cb == 0) return;
    hipLaunchKernelGGL((k_cb_forms_fill<IT, ROWS>), dim3(static_cast<unsigned>(sb + cb)), dim3(kCbFillThreads), 0, st, t, fm, uniq, uinfo,
                       static_cast<int32_t>(n_rows), rows, T, S_d, rank, form_of, sb, slot_form, static_cast<IT*>(chars));
}

bool cb_ids_ok(int64_t n_ids, int64_t Ne, int64_t S) {
    return n_ids >= 2 && n_ids <= kCbMaxIds && n_ids % 2 == 0 && Ne >= 0 && Ne < (int64_t{1} << 31) - 1 && S >= 1 && S < (int64_t{1} << 31);
}

// the host arrays of recon_ctx_batch_* -> the kernels' argument; false: a NULL table or a dimension out of range
bool cb_tables(const void* const* tables, const int64_t* dims, bool want_gat, CbTables* t) {
    if (!tables || !dims) return false;
    for (int i = 0; i < CB_T_GAT_ROW; ++i)
        if (!tables[i]) return false;
    if (want_gat && (!tables[CB_T_GAT_ROW] || !tables[CB_T_GAT_EMB] || dims[CB_D_G] < 1)) return false;
    if (dims[CB_D_MAX_T] < 1 || dims[CB_D_MAX_T] > 4096 || dims[CB_D_MAX_P] < 1 || dims[CB_D_MAX_P] > 4096 || dims[CB_D_MCL] < 1 || dims[CB_D_MCL] > 4096 ||
        dims[CB_D_CFS] < 1 || dims[CB_D_CFS] > 4096 || dims[CB_D_G] < 0 || dims[CB_D_G] >= (int64_t{1} << 30))
        return false;
    t->Ne = dims[CB_D_NE];
    t->S = dims[CB_D_S];
    t->max_T = static_cast<int32_t>(dims[CB_D_MAX_T]);
    t->max_P = static_cast<int32_t>(dims[CB_D_MAX_P]);
    t->mcl = static_cast<int32_t>(dims[CB_D_MCL]);
    t->cfs = static_cast<int32_t>(dims[CB_D_CFS]);
    t->pad = static_cast<int32_t>(dims[CB_D_PAD]);
    t->G = static_cast<int32_t>(dims[CB_D_G]);
    t->ent_line_ptr = static_cast<const int32_t*>(tables[CB_T_LINE_PTR]);
    t->ent_max_len = static_cast<const int32_t*>(tables[CB_T_MAX_LEN]);
    t->line_start = static_cast<const int32_t*>(tables[CB_T_LINE_START]);
    t->line_len = static_cast<const int32_t*>(tables[CB_T_LINE_LEN]);
    t->sf_start = static_cast<const int32_t*>(tables[CB_T_SF_START]);
    t->sf_len = static_cast<const int32_t*>(tables[CB_T_SF_LEN]);
    t->tok_flat = static_cast<const int32_t*>(tables[CB_T_FLAT]);
    t->tok_word = static_cast<const int32_t*>(tables[CB_T_WORD]);
    t->tok_chars = static_cast<const int32_t*>(tables[CB_T_CHARS]);
    t->gat_row = static_cast<const int32_t*>(tables[CB_T_GAT_ROW]);
    t->gat_emb = static_cast<const float*>(tables[CB_T_GAT_EMB]);
    return true;
}

// `n_rows` rows of either form (the padded form: U P_b, with the mask behind them)
template <typename IT, typename ROWS>
void cb_launch_fill(hipStream_t st, const CbTables& t, const int64_t* uniq, const int32_t* uinfo, int64_t n_rows, const ROWS& rows, int32_t T, void* words,
                    void* chars, void* mask, bool with_chars = true) {
    constexpr int VE = 16 / sizeof(IT);
    const int64_t W = t.cfs - 1 + static_cast<int64_t>(T) * (t.mcl + t.cfs - 1);
    const int32_t cs = static_cast<int32_t>((reinterpret_cast<uintptr_t>(chars) & 15u) / sizeof(IT));
    const int32_t ws = static_cast<int32_t>((reinterpret_cast<uintptr_t>(words) & 15u) / sizeof(IT));
    const int64_t cb = with_chars ? ceil_div64(ceil_div64(n_rows * W + cs, VE), kCbFillThreads) : 0;       // (the forms' batch has no char block)
    const int64_t wb = ceil_div64(ceil_div64(n_rows * T + ws, VE), kCbFillThreads);
    const int64_t mb = ROWS::kMask ? ceil_div64(n_rows, kCbFillThreads) : 0;
    hipLaunchKernelGGL((k_cb_fill<IT, ROWS>), dim3(static_cast<unsigned>(cb + wb + mb)), dim3(kCbFillThreads), 0, st, t, uniq, uinfo,
                       static_cast<int32_t>(n_rows), rows, T, static_cast<IT*>(words), static_cast<IT*>(chars), static_cast<uint8_t*>(mask), cb, wb, cs, ws);
}

// what recon_ctx_batch_fill and recon_ctx_batch_fill_ragged check alike, over n_rows rows
int cb_fill_args(const void* const* tables, const int64_t* dims, const int64_t* uniq, const int32_t* uinfo, int64_t U, int64_t n_rows, int32_t P_b, int32_t T_b,
                 int32_t index_bytes, const void* words, const void* chars, CbTables* t, bool with_chars = true) {
    if (U < 1 || P_b < 1 || T_b < 0 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (!cb_tables(tables, dims, false, t)) return RECON_ERR_INVALID;
    if (!uniq || !uinfo || (with_chars && !chars) || (T_b > 0 && !words)) return RECON_ERR_INVALID;
    if (P_b > t->max_P || T_b > t->max_T) return RECON_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(chars) | reinterpret_cast<uintptr_t>(words)) % static_cast<uintptr_t>(index_bytes)) return RECON_ERR_INVALID;
    if (U > kCbMaxIds + 1) return RECON_ERR_UNSUPPORTED;
    // every flat index of the char block, the last workgroup's past-the-end ones included, fits an int32
    if (static_cast<int64_t>(T_b) * (t->mcl + t->cfs - 1) > (int64_t{1} << 24) ||
        n_rows * (t->cfs - 1 + static_cast<int64_t>(T_b) * (t->mcl + t->cfs - 1)) >= kCbMaxCells)
        return RECON_ERR_UNSUPPORTED;
    return RECON_OK;
}

}  // namespace
}  // namespace recon

extern "C" int recon_ctx_batch_supported(int64_t n_ids, int64_t num_entities, int64_t num_surfaces) {
    return recon::cb_ids_ok(n_ids, num_entities, num_surfaces) ? 1 : 0;
}

extern "C" int recon_ctx_batch_index(const void* const* tables, const int64_t* dims, const int64_t* entity_indices, const int32_t* surface_ids,
                                     int64_t n_pairs, int32_t gat_mode, int64_t* unique_entities, int32_t* unique_info, int64_t* entities_position,
                                     int64_t* nonzero_entity_pos, int32_t* pair_slot, int32_t* header, recon_stream_t stream) {
    using namespace recon;
    if (n_pairs < 1 || gat_mode < 0 || gat_mode > 2) return RECON_ERR_INVALID;
    CbTables t;
    if (!cb_tables(tables, dims, gat_mode != 0, &t)) return RECON_ERR_INVALID;
    if (!entity_indices || !surface_ids || !unique_entities || !unique_info || !entities_position || !nonzero_entity_pos || !pair_slot || !header)
        return RECON_ERR_INVALID;
    if (n_pairs > kCbMaxIds / 2 || !cb_ids_ok(2 * n_pairs, t.Ne, t.S)) return RECON_ERR_UNSUPPORTED;
    const int32_t n = static_cast<int32_t>(2 * n_pairs);
    uint32_t H = 64;
    while (H < 2u * static_cast<uint32_t>(n) && H < static_cast<uint32_t>(kCbMaxIds)) H <<= 1;
    const size_t lds = (4 * static_cast<size_t>(H) + 2 * kCbWords + 8) * sizeof(uint32_t);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cb_index), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    hipLaunchKernelGGL(k_cb_index, dim3(1), dim3(kCbThreads), lds, as_stream(stream), t, entity_indices, surface_ids, n, H, gat_mode, unique_entities,
                       unique_info, entities_position, nonzero_entity_pos, pair_slot, header);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_ctx_batch_fill(const void* const* tables, const int64_t* dims, const int64_t* unique_entities, const int32_t* unique_info, int64_t U,
                                    int32_t P_b, int32_t T_b, int32_t index_bytes, void* context_words, void* context_chars, void* context_mask,
                                    recon_stream_t stream) {
    using namespace recon;
    CbTables t;
    if (U >= 1 && P_b >= 1 && !context_mask) return RECON_ERR_INVALID;
    const int rc = cb_fill_args(tables, dims, unique_entities, unique_info, U, U * P_b, P_b, T_b, index_bytes, context_words, context_chars, &t);
    if (rc != RECON_OK) return rc;
    const CbPaddedRows rows{P_b};
    if (index_bytes == 8) cb_launch_fill<int64_t>(as_stream(stream), t, unique_entities, unique_info, U * P_b, rows, T_b, context_words, context_chars, context_mask);
    else cb_launch_fill<int32_t>(as_stream(stream), t, unique_entities, unique_info, U * P_b, rows, T_b, context_words, context_chars, context_mask);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_ctx_batch_fill_ragged(const void* const* tables, const int64_t* dims, const int64_t* unique_entities, const int32_t* unique_info,
                                           int64_t U, int64_t L, int32_t P_b, int32_t T_b, int32_t index_bytes, void* context_words, void* context_chars,
                                           int32_t* line_ptr, int32_t* row_entity, recon_stream_t stream) {
    using namespace recon;
    CbTables t;
    if (L < U || (U >= 1 && P_b >= 1 && L > U * P_b) || !line_ptr || !row_entity) return RECON_ERR_INVALID;
    const int rc = cb_fill_args(tables, dims, unique_entities, unique_info, U, L, P_b, T_b, index_bytes, context_words, context_chars, &t);
    if (rc != RECON_OK) return rc;
    hipLaunchKernelGGL(k_cb_scan, dim3(1), dim3(kCbThreads), 0, as_stream(stream), unique_info, static_cast<int32_t>(U), P_b, static_cast<int32_t>(L),
                       line_ptr, row_entity);
    RECON_CHECK_LAUNCH();
    const CbRaggedRows rows{line_ptr, row_entity};
    if (index_bytes == 8) cb_launch_fill<int64_t>(as_stream(stream), t, unique_entities, unique_info, L, rows, T_b, context_words, context_chars, nullptr);
    else cb_launch_fill<int32_t>(as_stream(stream), t, unique_entities, unique_info, L, rows, T_b, context_words, context_chars, nullptr);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_ctx_batch_gat(const void* const* tables, const int64_t* dims, const int64_t* entity_indices, int64_t n_pairs, const int32_t* pair_slot,
                                   float* gat_entity_embeddings, float* nonzero_gat_entity_embeddings, recon_stream_t stream) {
    using namespace recon;
    if (n_pairs < 1) return RECON_ERR_INVALID;
    CbTables t;
    if (!cb_tables(tables, dims, true, &t)) return RECON_ERR_INVALID;
    if (!entity_indices || !gat_entity_embeddings || (nonzero_gat_entity_embeddings && !pair_slot)) return RECON_ERR_INVALID;
    if (n_pairs > kCbMaxIds / 2 || !cb_ids_ok(2 * n_pairs, t.Ne, t.S)) return RECON_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_cb_gat, dim3(static_cast<unsigned>(ceil_div64(n_pairs, kCbFillThreads / kWave))), dim3(kCbFillThreads), 0, as_stream(stream), t,
                       entity_indices, n_pairs, pair_slot, gat_entity_embeddings, nonzero_gat_entity_embeddings);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" size_t recon_ctx_batch_forms_scratch_bytes(int64_t num_forms) {
    if (num_forms < 1 || num_forms >= (int64_t{1} << 31) - recon::kCbFormTile) return 0;
    return static_cast<size_t>(3 * num_forms) * sizeof(int32_t);
}

extern "C" int recon_ctx_batch_forms_count(const void* const* tables, const int64_t* dims, const int32_t* tok_form, const int32_t* form_chars, int64_t num_forms,
                                           const int64_t* unique_entities, const int32_t* unique_info, int64_t n_pairs, int32_t ragged, int32_t* scratch,
                                           int32_t* header, recon_stream_t stream) {
    using namespace recon;
    if (n_pairs < 1 || n_pairs > kCbMaxIds / 2 || (ragged != 0 && ragged != 1)) return RECON_ERR_INVALID;
    CbTables t;
    CbForms fm;
    if (!cb_tables(tables, dims, false, &t) || !cb_forms(dims, tok_form, form_chars, num_forms, &fm)) return RECON_ERR_INVALID;
    if (!unique_entities || !unique_info || !scratch || !header) return RECON_ERR_INVALID;
    int32_t* flags = scratch;
    int32_t* rank = scratch + num_forms;
    int32_t* form_of = rank + num_forms;
    const hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(flags, 0, static_cast<size_t>(num_forms) * sizeof(int32_t), st) != hipSuccess) return RECON_ERR_LAUNCH;
    const int32_t max_U = static_cast<int32_t>(2 * n_pairs + 1);
    const int64_t blocks = std::min<int64_t>(1024, ceil_div64(static_cast<int64_t>(max_U) * t.max_P, kCbFillThreads));
    hipLaunchKernelGGL(k_cb_forms_mark, dim3(static_cast<unsigned>(blocks)), dim3(kCbFillThreads), 0, st, t, fm, unique_entities, unique_info, header, max_U,
                       ragged, flags);
    RECON_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_cb_forms_scan, dim3(1), dim3(kCbThreads), 0, st, flags, fm.NFm, rank, form_of, header);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_ctx_batch_fill_forms(const void* const* tables, const int64_t* dims, const int32_t* tok_form, const int32_t* form_chars, int64_t num_forms,
                                          const int32_t* scratch, const int64_t* unique_entities, const int32_t* unique_info, int64_t U, int64_t n_rows,
                                          int32_t P_b, int32_t T_b, int64_t S_d, int32_t ragged, int32_t index_bytes, void* context_words, void* context_mask,
                                          int32_t* line_ptr, int32_t* row_entity, void* form_rows, int32_t* slot_form, recon_stream_t stream) {
    using namespace recon;
    CbTables t;
    CbForms fm;
    if (ragged != 0 && ragged != 1) return RECON_ERR_INVALID;
    if (ragged ? (n_rows < U || (U >= 1 && P_b >= 1 && n_rows > U * P_b) || !line_ptr || !row_entity) : (n_rows != U * P_b || !context_mask)) return RECON_ERR_INVALID;
    const int rc = cb_fill_args(tables, dims, unique_entities, unique_info, U, n_rows, P_b, T_b, index_bytes, context_words, nullptr, &t, false);
    if (rc != RECON_OK) return rc;
    if (!cb_forms(dims, tok_form, form_chars, num_forms, &fm) || !scratch) return RECON_ERR_INVALID;
    const int64_t n_slots = n_rows * T_b;
    if (S_d < 0 || S_d > num_forms || S_d > n_slots || (n_slots > 0 && S_d < 1)) return RECON_ERR_INVALID;
    if ((n_slots > 0 && !slot_form) || (S_d > 0 && !form_rows)) return RECON_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(form_rows) % static_cast<uintptr_t>(index_bytes)) return RECON_ERR_INVALID;
    const int32_t* rank = scratch + num_forms;
    const int32_t* form_of = rank + num_forms;
    const hipStream_t st = as_stream(stream);
    const int32_t s_d = static_cast<int32_t>(S_d);
    if (ragged) {
        hipLaunchKernelGGL(k_cb_scan, dim3(1), dim3(kCbThreads), 0, st, unique_info, static_cast<int32_t>(U), P_b, static_cast<int32_t>(n_rows), line_ptr, row_entity);
        RECON_CHECK_LAUNCH();
        const CbRaggedRows rows{line_ptr, row_entity};
        if (index_bytes == 8) {
            cb_launch_fill<int64_t>(st, t, unique_entities, unique_info, n_rows, rows, T_b, context_words, nullptr, nullptr, false);
            cb_launch_forms_fill<int64_t>(st, t, fm, unique_entities, unique_info, n_rows, rows, T_b, s_d, rank, form_of, slot_form, form_rows);
        } else {
            cb_launch_fill<int32_t>(st, t, unique_entities, unique_info, n_rows, rows, T_b, context_words, nullptr, nullptr, false);
            cb_launch_forms_fill<int32_t>(st, t, fm, unique_entities, unique_info, n_rows, rows, T_b, s_d, rank, form_of, slot_form, form_rows);
        }
    } else {
        const CbPaddedRows rows{P_b};
        if (index_bytes == 8) {
            cb_launch_fill<int64_t>(st, t, unique_entities, unique_info, n_rows, rows, T_b, context_words, nullptr, context_mask, false);
            cb_launch_forms_fill<int64_t>(st, t, fm, unique_entities, unique_info, n_rows, rows, T_b, s_d, rank, form_of, slot_form, form_rows);
        } else {
            cb_launch_fill<int32_t>(st, t, unique_entities, unique_info, n_rows, rows, T_b, context_words, nullptr, context_mask, false);
            cb_launch_forms_fill<int32_t>(st, t, fm, unique_entities, unique_info, n_rows, rows, T_b, s_d, rank, form_of, slot_form, form_rows);
        }
    }
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}
