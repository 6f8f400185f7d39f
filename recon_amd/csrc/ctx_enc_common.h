// What the entity-context ops (char_cnn.hip, char_mask.hip, ctx_lstm.hip) share on both sides of a launch, said once.  Their kernels, launch
// bounds, grids, LDS sizes and k* constants stay in their own files; the constants come in here as arguments.
#pragma once
#include <initializer_list>
#include <type_traits>
#include "recon_common.h"

namespace recon {

typedef float enc_f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// id j of the word at `cp` in lane j (j < n), clamped into the table: an id outside [0, V) is the caller's error, never an access outside
template <typename IdT>
__device__ __forceinline__ int word_ids(const IdT* cp, int lane, int n, int V) {
    int64_t v = 0;
    if (lane < n) v = static_cast<int64_t>(cp[lane]);
    return static_cast<int>(v < 0 ? 0 : (v >= V ? V - 1 : v));
}

// true when `kern` may be launched with `lds` bytes of dynamic LDS (above 48 KiB the runtime has to be asked)
template <typename K>
bool allow_lds(K kern, size_t lds) {
    return lds <= 48 * 1024 ||
           hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) == hipSuccess;
}

// workgroups of a pass that sums over n rows and the rows each owns, per = max(ceil(n / max_wg), min_per): a function of the shape alone
// (the summation order must not change between runs)
inline void split_rows(int64_t n, int64_t max_wg, int64_t min_per, int64_t* per, int32_t* G) {
    int64_t p = ceil_div64(n, max_wg);
    if (p < min_per) p = min_per;
    *per = p;
    *G = static_cast<int32_t>(ceil_div64(n, p));
}

// the parameter gradients of an empty batch: every output zeroed on the stream, in list order
struct ZeroFill { float* p; size_t floats; };
inline int zero_fill(std::initializer_list<ZeroFill> outs, hipStream_t st) {
    for (const ZeroFill& o : outs)
        if (hipMemsetAsync(o.p, 0, o.floats * 4, st) != hipSuccess) return RECON_ERR_LAUNCH;
    return RECON_OK;
}

// (index_bytes, lds) -> the <LDS, IdT> instance of a launch: f(std::bool_constant<LDS>, IdTag<IdT>) names its argument list once
template <typename T> struct IdTag { using type = T; };
template <typename F>
int dispatch_lds_ids(int32_t index_bytes, bool lds, F&& f) {
    if (index_bytes == 8) return lds ? f(std::true_type{}, IdTag<int64_t>{}) : f(std::false_type{}, IdTag<int64_t>{});
    return lds ? f(std::true_type{}, IdTag<int32_t>{}) : f(std::false_type{}, IdTag<int32_t>{});
}
// the same for kernels without an LDS form: f(IdTag<IdT>)
template <typename F>
int dispatch_ids(int32_t index_bytes, F&& f) {
    return dispatch_lds_ids(index_bytes, false, [&](auto, auto id) { return f(id); });
}

// what the four char entries check once the shape is accepted: every pointer there (the caller's `have_all`), the id rows long enough, the
// workspace aligned and of `need` bytes
inline int char_io_checks(bool have_all, int64_t ld_chars, int32_t W, int32_t span, int32_t cfs, const void* workspace, size_t workspace_bytes,
                          size_t need) {
    if (!have_all || ld_chars < cfs - 1 + static_cast<int64_t>(W) * span) return RECON_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return RECON_ERR_INVALID;
    if (workspace_bytes < need) return RECON_ERR_WORKSPACE;
    return RECON_OK;
}

}  // namespace recon
