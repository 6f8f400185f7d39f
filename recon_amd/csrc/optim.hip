// Parameter updates of the three training programs as multi-tensor kernels: SGD (GAT/main.py:445-449), Adam with L2 weight decay
// (GAT/main.py:747-751, train.py:234) and the global gradient norm of clip_grad_norm (train.py:314-315) in front of either.
//
// One launch covers up to kOptMaxSegs (parameter, gradient, state) segments of any sizes.  The segment descriptors — pointers, element
// counts and the cumulative count of kOptChunk-element chunks — travel IN THE KERNEL ARGUMENTS (2.6 KB of HIP's 4 KB for Adam's four
// pointers per segment): no device table, no copy, nothing to rebuild when autograd hands over gradients at new addresses.  Workgroup b
// owns chunk b of the launch; it finds its segment with one 64-lane compare of b against the cumulative counts and a ballot.
//
// Memory access: a chunk whose pointers are all 16-byte aligned moves 16 bytes per lane (its offset inside the segment is a multiple of
// kOptChunk floats, so the segment bases decide); any other chunk — a gradient that is a view into a flat bucket at an arbitrary float
// offset — moves 4 bytes per lane.  The choice is made per chunk from the addresses: it is uniform over the workgroup.  Every load of
// a thread is issued before its first store (the buffers of a segment must not overlap each other).
//
// k_optim_sumsq: every workgroup leaves the sum of squares of its chunk, accumulated in fp64, in its own word of the workspace; the
//   workgroup that arrives last at the launch's counter adds ALL words in index order (fp64) and writes total_norm = sqrt(sum) and the
//   clip scale min(1, max_norm / (total_norm + 1e-6)) (torch.nn.utils.clip_grad_norm_'s formula, evaluated in fp32 like there).  Which
//   workgroup arrives last changes who adds, never the order of the additions: the same inputs give the same bits.  The words are
//   handed over by agent-scope atomic stores and loads and an acquire-release add on the counter; nobody waits for anybody.
#include "recon_common.h"

#include <math.h>
#include <initializer_list>

namespace recon {
namespace {

constexpr int kOptThreads = 256;
constexpr int kOptPer = 16;                                  // elements per thread: four 16-byte accesses
constexpr int kOptChunk = kOptThreads * kOptPer;             // 4096 elements per workgroup
constexpr int kOptMaxSegs = 64;                              // = lanes of a wave (the segment search is one compare per lane)
constexpr int64_t kOptMaxSegElems = int64_t(1) << 30;        // longer segments are cut at a chunk boundary by the host code below
static_assert(kOptMaxSegs == kWave && kOptMaxSegElems % kOptChunk == 0, "segment search / segment cut");

// NP pointers per segment: 1 = gradient (sum of squares), 2 = parameter, gradient (SGD), 4 = parameter, gradient, exp_avg, exp_avg_sq (Adam)
template <int NP>
struct OptSegs {
    float* ptr[NP][kOptMaxSegs];
    int32_t n[kOptMaxSegs];
    uint32_t chunk_end[kOptMaxSegs];                         // chunks of segments 0 .. i (entries past the last segment repeat the total)
};
static_assert(sizeof(OptSegs<4>) + 64 <= 4096, "kernel arguments");

// this workgroup's chunk: segment index, element offset inside the segment, elements (1 .. kOptChunk)
struct OptChunk { int seg; int64_t off; int cnt; };

template <int NP>
__device__ __forceinline__ OptChunk opt_find_chunk(const OptSegs<NP>& S) {
    const uint32_t b = blockIdx.x;
    const unsigned long long past = __ballot(b >= S.chunk_end[threadIdx.x & 63]);      // every wave of the workgroup computes the same
    const int seg = __builtin_amdgcn_readfirstlane(__popcll(past));
    const uint32_t first = seg ? S.chunk_end[seg - 1] : 0u;
    OptChunk c;
    c.seg = seg;
    c.off = static_cast<int64_t>(b - first) * kOptChunk;
    const int64_t left = S.n[seg] - c.off;
    c.cnt = static_cast<int>(left < kOptChunk ? left : kOptChunk);
    return c;
}

__device__ __forceinline__ bool opt_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15u) == 0;
}

// Element slots of a thread.  VEC: slot j holds elements 4 (256 j + t) .. + 3, whole float4s only; the cnt % 4 elements behind the last
// whole float4 are slot kOptPer / 4 of threads 0 .. cnt % 4 - 1.  Scalar: slot j holds element 256 j + t.  FULL: the chunk has all its
// kOptChunk elements — every slot is live and there is no tail, so nothing stands between the loads (a condition around a load makes
// hipcc branch around it and wait for it alone); every chunk of a segment but its last takes this form.
template <bool VEC, bool FULL>
struct OptWalk {
    static constexpr int kSlots = VEC ? kOptPer / 4 : kOptPer;
    static constexpr int kWidth = VEC ? 4 : 1;
    __device__ static __forceinline__ int index(int j, int t) { return kWidth * (kOptThreads * j + t); }
    __device__ static __forceinline__ bool live(int j, int t, int cnt) { return FULL || index(j, t) + kWidth <= cnt; }
    __device__ static __forceinline__ int tail(int t, int cnt) { return FULL ? cnt : VEC ? (cnt & ~3) + t : cnt; }   // < cnt: thread t owns it
};

// The arithmetic is written in the operation order of torch's single-tensor fp32 implementations (torch/optim/sgd.py, adam.py over ATen's
// CPU kernels) with contraction switched off, so that each rounding here has its counterpart there: add(alpha) and lerp are one fma,
// mul / addcmul / sqrt / div / addcdiv round after every operation.  exp_avg in particular is m + (1 - beta1) (g' - m), not
// beta1 m + (1 - beta1) g': in fp32 the decay 1 - fl(0.1) is 16 times closer to 0.9 than fl(0.9) is, and that error compounds per step.
struct SgdOp {
    float neg_lr, wd, s;
    __device__ __forceinline__ void operator()(float& p, float g) const {
#pragma clang fp contract(off)
        float gp = s * g;                                                  // clip_grad_norm_: g.mul_(clip_coef)
        if (wd != 0.f) gp = fmaf(wd, p, gp);                               // grad.add(param, alpha=weight_decay)
        p = fmaf(neg_lr, gp, p);                                           // param.add_(grad, alpha=-lr)
    }
};

struct AdamOp {
    float neg_step_size, omb1, b2, omb2, bc2_sqrt, eps, wd, s;
    __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v) const {
#pragma clang fp contract(off)
        float gp = s * g;
        if (wd != 0.f) gp = fmaf(wd, p, gp);
        m = fmaf(omb1, gp - m, m);                                         // exp_avg.lerp_(grad, 1 - beta1)
        v = v * b2 + (omb2 * gp) * gp;                                     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        const float denom = sqrtf(v) / bc2_sqrt + eps;                     // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
        p = p + (neg_step_size * m) / denom;                               // param.addcdiv_(exp_avg, denom, value=-step_size)
    }
};

template <bool VEC, bool FULL, class Op>
__device__ __forceinline__ void sgd_chunk(float* __restrict__ p, const float* __restrict__ g, int cnt, const Op& op) {
    using W = OptWalk<VEC, FULL>;
    const int t = threadIdx.x;
    float pv[W::kSlots][W::kWidth], gv[W::kSlots][W::kWidth];
#pragma unroll
    for (int j = 0; j < W::kSlots; ++j)
        if (W::live(j, t, cnt)) { load_vec<W::kWidth>(pv[j], p + W::index(j, t)); load_vec<W::kWidth>(gv[j], g + W::index(j, t)); }
    const int tail = W::tail(t, cnt);
    float pt = 0.f, gt = 0.f;
    if (tail < cnt) { pt = p[tail]; gt = g[tail]; }
#pragma unroll
    for (int j = 0; j < W::kSlots; ++j)
        if (W::live(j, t, cnt)) {
#pragma unroll
            for (int e = 0; e < W::kWidth; ++e) op(pv[j][e], gv[j][e]);
            store_vec<W::kWidth>(p + W::index(j, t), pv[j]);
        }
    if (tail < cnt) { op(pt, gt); p[tail] = pt; }
}

template <bool VEC, bool FULL, class Op>
__device__ __forceinline__ void adam_chunk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int cnt,
                                           const Op& op) {
    using W = OptWalk<VEC, FULL>;
    const int t = threadIdx.x;
    float pv[W::kSlots][W::kWidth], gv[W::kSlots][W::kWidth], mv[W::kSlots][W::kWidth], vv[W::kSlots][W::kWidth];
#pragma unroll
    for (int j = 0; j < W::kSlots; ++j)
        if (W::live(j, t, cnt)) {
            const int i = W::index(j, t);
            load_vec<W::kWidth>(pv[j], p + i); load_vec<W::kWidth>(gv[j], g + i); load_vec<W::kWidth>(mv[j], m + i); load_vec<W::kWidth>(vv[j], v + i);
        }
    const int tail = W::tail(t, cnt);
    float pt = 0.f, gt = 0.f, mt = 0.f, vt = 0.f;
    if (tail < cnt) { pt = p[tail]; gt = g[tail]; mt = m[tail]; vt = v[tail]; }
#pragma unroll
    for (int j = 0; j < W::kSlots; ++j)
        if (W::live(j, t, cnt)) {
            const int i = W::index(j, t);
#pragma unroll
            for (int e = 0; e < W::kWidth; ++e) op(pv[j][e], gv[j][e], mv[j][e], vv[j][e]);
            store_vec<W::kWidth>(p + i, pv[j]); store_vec<W::kWidth>(m + i, mv[j]); store_vec<W::kWidth>(v + i, vv[j]);
        }
    if (tail < cnt) { op(pt, gt, mt, vt); p[tail] = pt; m[tail] = mt; v[tail] = vt; }
}

__global__ void __launch_bounds__(kOptThreads) k_optim_sgd(const OptSegs<2> S, float lr, float wd, const float* __restrict__ scale) {
    const OptChunk c = opt_find_chunk(S);
    float* p = S.ptr[0][c.seg] + c.off;
    const float* g = S.ptr[1][c.seg] + c.off;
    const SgdOp op{-lr, wd, scale ? *scale : 1.f};
    const bool vec = opt_aligned16(p, g), full = c.cnt == kOptChunk;
    if (vec && full) sgd_chunk<true, true>(p, g, c.cnt, op);
    else if (vec) sgd_chunk<true, false>(p, g, c.cnt, op);
    else if (full) sgd_chunk<false, true>(p, g, c.cnt, op);
    else sgd_chunk<false, false>(p, g, c.cnt, op);
}

__global__ void __launch_bounds__(kOptThreads) k_optim_adam(const OptSegs<4> S, float step_size, float omb1, float b2, float omb2,
                                                            float bc2_sqrt, float eps, float wd, const float* __restrict__ scale) {
    const OptChunk c = opt_find_chunk(S);
    float* p = S.ptr[0][c.seg] + c.off;
    const float* g = S.ptr[1][c.seg] + c.off;
    float* m = S.ptr[2][c.seg] + c.off;
    float* v = S.ptr[3][c.seg] + c.off;
    const AdamOp op{-step_size, omb1, b2, omb2, bc2_sqrt, eps, wd, scale ? *scale : 1.f};
    const bool vec = opt_aligned16(p, g, m, v), full = c.cnt == kOptChunk;
    if (vec && full) adam_chunk<true, true>(p, g, m, v, c.cnt, op);
    else if (vec) adam_chunk<true, false>(p, g, m, v, c.cnt, op);
    else if (full) adam_chunk<false, true>(p, g, m, v, c.cnt, op);
    else adam_chunk<false, false>(p, g, m, v, c.cnt, op);
}

// ---- global gradient norm ----------------------------------------------------------------------------------------------------------
// workspace: [0] total_norm (fp32)  [1] clip scale (fp32)  [2] arrival counter (uint32, zero between launches)  [3] unused
//            byte 16 onwards: one fp64 word per chunk of the step, as 64-bit patterns
constexpr size_t kOptWsHeader = 16;
using opt_u64 = unsigned long long;

// sum over the workgroup in one fixed order; the total arrives in thread 0
__device__ __forceinline__ double opt_block_sum(double a, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    const int t = threadIdx.x;
    if ((t & 63) == 0) red[t >> 6] = a;
    __syncthreads();
    double tot = 0.0;
    if (t == 0)
        for (int w = 0; w < kOptThreads / 64; ++w) tot += red[w];
    return tot;
}

template <bool VEC, bool FULL>
__device__ __forceinline__ double sumsq_chunk(const float* __restrict__ g, int cnt) {
    using W = OptWalk<VEC, FULL>;
    const int t = threadIdx.x;
    float gv[W::kSlots][W::kWidth];
#pragma unroll
    for (int j = 0; j < W::kSlots; ++j) {
#pragma unroll
        for (int e = 0; e < W::kWidth; ++e) gv[j][e] = 0.f;
        if (W::live(j, t, cnt)) load_vec<W::kWidth>(gv[j], g + W::index(j, t));
    }
    const int tail = W::tail(t, cnt);
    const float gt = tail < cnt ? g[tail] : 0.f;
    double a = static_cast<double>(gt) * gt;
#pragma unroll
    for (int j = 0; j < W::kSlots; ++j)
#pragma unroll
        for (int e = 0; e < W::kWidth; ++e) a = fma(static_cast<double>(gv[j][e]), static_cast<double>(gv[j][e]), a);
    return a;
}

// `words`: this launch's first word; `all_words` / `n_words`: every word of the step (only the step's LAST launch, finish != 0, reads them:
// the launches in front of it have completed, their words are plain memory by then)
__global__ void __launch_bounds__(kOptThreads) k_optim_sumsq(const OptSegs<1> S, opt_u64* words, opt_u64* all_words, uint32_t n_words, int finish,
                                                             float max_norm, float* out, uint32_t* counter) {
    __shared__ double red[kOptThreads / 64];
    __shared__ int is_last;
    const OptChunk c = opt_find_chunk(S);
    const float* g = S.ptr[0][c.seg] + c.off;
    const bool vec = opt_aligned16(g), full = c.cnt == kOptChunk;
    const double part = vec ? (full ? sumsq_chunk<true, true>(g, c.cnt) : sumsq_chunk<true, false>(g, c.cnt))
                            : (full ? sumsq_chunk<false, true>(g, c.cnt) : sumsq_chunk<false, false>(g, c.cnt));
    const double tot = opt_block_sum(part, red);
    const int t = threadIdx.x;
    if (t == 0) {
        __hip_atomic_store(words + blockIdx.x, __builtin_bit_cast(opt_u64, tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int last = 0;
        if (finish) last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
        is_last = last;
    }
    __syncthreads();
    if (!is_last) return;
    double a = 0.0;
    for (uint32_t i = t; i < n_words; i += kOptThreads)
        a += __builtin_bit_cast(double, __hip_atomic_load(all_words + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    __syncthreads();                                                      // red[] is reused
    const double sum = opt_block_sum(a, red);
    if (t == 0) {
        const float norm = static_cast<float>(sqrt(sum));
        const float coef = max_norm / (norm + 1e-6f);
        out[0] = norm;
        out[1] = coef > 1.f ? 1.f : coef;                                 // (a NaN stays a NaN, as torch.clamp keeps it)
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- host side: the caller's segment lists -> launches of at most kOptMaxSegs segments ------------------------------------------------
template <int NP>
struct OptBatcher {
    OptSegs<NP> S;
    int nseg = 0;
    uint32_t chunks = 0;
    bool full() const { return nseg == kOptMaxSegs; }
    void add(float* const (&ptr)[NP], int64_t off, int32_t n) {
        for (int q = 0; q < NP; ++q) S.ptr[q][nseg] = ptr[q] + off;
        S.n[nseg] = n;
        chunks += static_cast<uint32_t>((n + kOptChunk - 1) / kOptChunk);
        S.chunk_end[nseg++] = chunks;
    }
    void seal() {                                                         // what the segment search reads past the last segment
        for (int i = nseg; i < kOptMaxSegs; ++i) {
            for (int q = 0; q < NP; ++q) S.ptr[q][i] = nullptr;
            S.n[i] = 0;
            S.chunk_end[i] = chunks;
        }
    }
    void reset() { nseg = 0; chunks = 0; }
};

// -1 / 0 / 1: invalid, nothing to do, work (the checks every entry point makes before its first launch)
int opt_check(int32_t n_segments, const int64_t* numel, std::initializer_list<const void*> arrays) {
    if (n_segments < 0) return -1;
    if (n_segments == 0) return 0;
    if (!numel) return -1;
    for (const void* a : arrays)
        if (!a) return -1;
    bool any = false;
    for (int32_t i = 0; i < n_segments; ++i) {
        if (numel[i] < 0) return -1;
        any = any || numel[i] > 0;
    }
    return any ? 1 : 0;
}

// walks the non-empty segments in pieces of at most kOptMaxSegElems elements, kOptMaxSegs pieces per launch; launch(batcher, last)
template <int NP, class Ptrs, class Launch>
int opt_for_each_launch(int32_t n_segments, const int64_t* numel, Ptrs ptrs, Launch launch) {
    for (int32_t i = 0; i < n_segments; ++i)
        for (int q = 0; q < NP; ++q)
            if (numel[i] > 0 && !ptrs(q, i)) return RECON_ERR_INVALID;
    OptBatcher<NP> b;
    for (int32_t i = 0; i < n_segments; ++i) {
        float* ptr[NP];
        for (int q = 0; q < NP; ++q) ptr[q] = ptrs(q, i);
        for (int64_t off = 0; off < numel[i]; off += kOptMaxSegElems) {
            if (b.full()) {
                b.seal();
                if (int rc = launch(b, false)) return rc;
                b.reset();
            }
            const int64_t left = numel[i] - off;
            b.add(ptr, off, static_cast<int32_t>(left < kOptMaxSegElems ? left : kOptMaxSegElems));
        }
    }
    b.seal();
    return launch(b, true);
}

}  // namespace
}  // namespace recon

extern "C" int32_t recon_optim_max_segments(void) { return recon::kOptMaxSegs; }
extern "C" int32_t recon_optim_chunk_elems(void) { return recon::kOptChunk; }

extern "C" size_t recon_optim_workspace_bytes(int64_t total_elems, int32_t n_segments) {
    if (total_elems < 0 || n_segments < 0) return 0;
    // a segment of n elements has ceil(n / chunk) <= n / chunk + 1 chunks; a cut of a long segment falls on a chunk boundary
    return recon::kOptWsHeader + (static_cast<size_t>(total_elems / recon::kOptChunk) + static_cast<size_t>(n_segments)) * sizeof(double);
}

extern "C" int recon_optim_grad_sumsq(const void* const* grads, const int64_t* numel, int32_t n_segments, float max_norm, void* workspace,
                                      size_t workspace_bytes, recon_stream_t stream) {
    using namespace recon;
    const int chk = opt_check(n_segments, numel, {grads});
    if (chk <= 0) return chk < 0 ? RECON_ERR_INVALID : RECON_OK;          // nothing to add up: the workspace is left as it is
    if (!workspace) return RECON_ERR_INVALID;
    int64_t total = 0;
    for (int32_t i = 0; i < n_segments; ++i) total += numel[i];
    if (workspace_bytes < recon_optim_workspace_bytes(total, n_segments)) return RECON_ERR_WORKSPACE;
    float* out = static_cast<float*>(workspace);
    uint32_t* counter = reinterpret_cast<uint32_t*>(workspace) + 2;
    opt_u64* words = reinterpret_cast<opt_u64*>(static_cast<char*>(workspace) + kOptWsHeader);
    hipStream_t st = as_stream(stream);
    uint32_t done = 0;
    return opt_for_each_launch<1>(n_segments, numel, [&](int, int32_t i) { return static_cast<float*>(const_cast<void*>(grads[i])); },
                                  [&](const OptBatcher<1>& b, bool last) {
                                      hipLaunchKernelGGL(k_optim_sumsq, dim3(b.chunks), dim3(kOptThreads), 0, st, b.S, words + done, words,
                                                         done + b.chunks, last ? 1 : 0, max_norm, out, counter);
                                      done += b.chunks;
                                      return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
                                  });
}

extern "C" int recon_optim_sgd(void* const* params, const void* const* grads, const int64_t* numel, int32_t n_segments, double lr,
                               double weight_decay, const float* clip_scale, recon_stream_t stream) {
    using namespace recon;
    const int chk = opt_check(n_segments, numel, {params, grads});
    if (chk <= 0) return chk < 0 ? RECON_ERR_INVALID : RECON_OK;
    hipStream_t st = as_stream(stream);
    return opt_for_each_launch<2>(n_segments, numel,
                                  [&](int q, int32_t i) { return static_cast<float*>(q == 0 ? params[i] : const_cast<void*>(grads[i])); },
                                  [&](const OptBatcher<2>& b, bool) {
                                      hipLaunchKernelGGL(k_optim_sgd, dim3(b.chunks), dim3(kOptThreads), 0, st, b.S, static_cast<float>(lr),
                                                         static_cast<float>(weight_decay), clip_scale);
                                      return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
                                  });
}

extern "C" int recon_optim_adam(void* const* params, const void* const* grads, void* const* exp_avg, void* const* exp_avg_sq,
                                const int64_t* numel, int32_t n_segments, double lr, double beta1, double beta2, double eps, double weight_decay,
                                double bias_correction1, double bias_correction2, const float* clip_scale, recon_stream_t stream) {
    using namespace recon;
    const int chk = opt_check(n_segments, numel, {params, grads, exp_avg, exp_avg_sq});
    if (chk < 0 || !(bias_correction1 > 0.0) || !(bias_correction2 > 0.0)) return RECON_ERR_INVALID;
    if (chk == 0) return RECON_OK;
    hipStream_t st = as_stream(stream);
    const float step_size = static_cast<float>(lr / bias_correction1), bc2_sqrt = static_cast<float>(sqrt(bias_correction2));
    return opt_for_each_launch<4>(n_segments, numel,
                                  [&](int q, int32_t i) {
                                      return static_cast<float*>(q == 0 ? params[i] : q == 1 ? const_cast<void*>(grads[i]) : q == 2 ? exp_avg[i] : exp_avg_sq[i]);
                                  },
                                  [&](const OptBatcher<4>& b, bool) {
                                      hipLaunchKernelGGL(k_optim_adam, dim3(b.chunks), dim3(kOptThreads), 0, st, b.S, step_size,
                                                         static_cast<float>(1.0 - beta1), static_cast<float>(beta2),
                                                         static_cast<float>(1.0 - beta2), bc2_sqrt, static_cast<float>(eps),
                                                         static_cast<float>(weight_decay), clip_scale);
                                      return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
                                  });
}
