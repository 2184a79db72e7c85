// The optimizer step of the training loop (include/ns2hip_optim.h): gradient norm + clip, Adam, EMA.  Reference: Trainer.train,
// NS2:1888-1901 (clip_grad_norm_, Adam.step(), ema.update()).  Plain streaming kernels: one workgroup per chunk of NS2_OPTIM_CHUNK
// values of one tensor, 16 bytes per lane and access where the tensor's arrays share their address modulo 16, no atomics, every
// reduction in a fixed order over fixed slots.  Device scalars (the state block) are written by one lane with ordinary stores.
// This translation unit converts nothing to half, so it includes no ns2_common.h and owns no range counter; it READS the others'.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/ns2hip_optim.h"
#include "ns2_host.h"

namespace ns2 {
namespace {

constexpr int OPT_THREADS = 256;                 // lanes per chunk: NS2_OPTIM_CHUNK / (4 * 256) = 4 rounds of 16-byte accesses
constexpr int FIN_THREADS = 256;                 // the finish workgroup
constexpr int W_MARKED = NS2_OPTIM_W_PRIVATE;    // (int) ns2_optim_mark has run
constexpr int W_NCOUNTERS = W_MARKED + 1;        // (int) registered range counters
constexpr int W_SNAP = 12;                       // their values at the last mark, SAT_COUNTERS_MAX words
constexpr int W_ADDR = W_SNAP + SAT_COUNTERS_MAX;   // their device addresses, SAT_COUNTERS_MAX 64-bit words (8-byte aligned: W_ADDR is even)
static_assert(W_NCOUNTERS < W_SNAP && W_ADDR % 2 == 0 && W_ADDR + 2 * SAT_COUNTERS_MAX <= NS2_OPTIM_STATE_WORDS, "state block layout");
static_assert(NS2_OPTIM_CHUNK % (4 * OPT_THREADS) == 0, "a chunk is whole rounds of 16-byte accesses");

struct OptChunk { int64_t start; int tensor; int len; };     // values [start, start + len) of tensor `tensor`, len <= NS2_OPTIM_CHUNK
static_assert(sizeof(OptChunk) == 16 && sizeof(ns2_optim_tensor) == 48, "table layout");

inline int64_t chunks_of(int64_t numel) { return (numel + NS2_OPTIM_CHUNK - 1) / NS2_OPTIM_CHUNK; }
inline int64_t off_chunks(int n) { return (int64_t)n * (int64_t)sizeof(ns2_optim_tensor); }
inline int64_t off_partials(int n, int64_t chunks) { return off_chunks(n) + chunks * (int64_t)sizeof(OptChunk); }

__device__ __forceinline__ unsigned low4(const void* p) { return (unsigned)((uintptr_t)p & 15u); }
// values before the first 16-byte boundary of a (4-byte aligned) address
__device__ __forceinline__ int head_of(unsigned low, int len) { return min(len, (int)(((16u - low) & 15u) >> 2)); }

// ---------------------------------------------------------------------------------------------------------------- norm
__global__ __launch_bounds__(OPT_THREADS) void optim_norm_kernel(const ns2_optim_tensor* __restrict__ tensors,
                                                                 const OptChunk* __restrict__ chunks, float* __restrict__ partial) {
  const OptChunk c = chunks[blockIdx.x];
  const float* g = tensors[c.tensor].grad;
  const int t = threadIdx.x;
  float acc = 0.f;
  if (g) {
    g += c.start;
    const int head = head_of(low4(g), c.len);
    const int nv = (c.len - head) >> 2, tail0 = head + 4 * nv;
    const float4* gv = reinterpret_cast<const float4*>(g + head);
    for (int i = t; i < nv; i += OPT_THREADS) {
      const float4 x = gv[i];
      acc += x.x * x.x; acc += x.y * x.y; acc += x.z * x.z; acc += x.w * x.w;
    }
    if (t < head) acc += g[t] * g[t];                            // up to 3 values in front of the first boundary
    if (t < c.len - tail0) acc += g[tail0 + t] * g[tail0 + t];   // ... and up to 3 behind the last one
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ float s[OPT_THREADS / 64];
  if ((t & 63) == 0) s[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    float tot = s[0];
    for (int w = 1; w < OPT_THREADS / 64; ++w) tot += s[w];
    partial[blockIdx.x] = tot;                                   // every chunk writes its slot every step (0 for a null grad)
  }
}

// ---------------------------------------------------------------------------------------------------------------- finish
__global__ __launch_bounds__(FIN_THREADS) void optim_finish_kernel(const float* __restrict__ partial, int64_t chunks, uint32_t* state,
                                                                   double beta1, double beta2, double max_grad_norm, int ema_every) {
  __shared__ double s[FIN_THREADS];
  const int t = threadIdx.x;
  double a = 0.0;
  for (int64_t i = t; i < chunks; i += FIN_THREADS) a += (double)partial[i];
  s[t] = a;
  __syncthreads();
  for (int w = FIN_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) s[t] += s[t + w];
    __syncthreads();
  }
  if (t != 0) return;
  float* f = reinterpret_cast<float*>(state);
  int* iw = reinterpret_cast<int*>(state);
  const float norm = (float)sqrt(s[0]);
  const float coef = max_grad_norm > 0.0 ? fminf(1.0f, (float)max_grad_norm / (norm + 1e-6f)) : 1.0f;   // clip_grad_norm_'s, in fp32
  int skip = isfinite(norm) ? 0 : 1;
  if (iw[W_MARKED]) {
    const volatile unsigned int* const* addr = reinterpret_cast<const volatile unsigned int* const*>(state + W_ADDR);
    for (int i = 0; i < iw[W_NCOUNTERS]; ++i)
      if (*addr[i] != state[W_SNAP + i]) skip = 1;               // != : a counter that was read and zeroed in between moved too
  }
  f[NS2_OPTIM_W_GRAD_NORM] = norm;
  f[NS2_OPTIM_W_CLIP_COEF] = coef;
  iw[NS2_OPTIM_W_SKIP] = skip;
  if (skip) return;
  const int step = iw[NS2_OPTIM_W_STEP] + 1;
  iw[NS2_OPTIM_W_STEP] = step;
  f[NS2_OPTIM_W_STEP_SIZE] = (float)((double)f[NS2_OPTIM_W_LR] / (1.0 - pow(beta1, (double)step)));
  f[NS2_OPTIM_W_BC2_SQRT] = (float)sqrt(1.0 - pow(beta2, (double)step));
  iw[NS2_OPTIM_W_EMA_DUE] = (ema_every > 0 && step % ema_every == 0) ? 1 : 0;
  f[NS2_OPTIM_W_EMA_WEIGHT] = (float)(1.0 - (double)f[NS2_OPTIM_W_EMA_DECAY]);
}

// ---------------------------------------------------------------------------------------------------------------- update
struct AdamK { float clip, omb1, beta2, omb2, eps, step_size, bc2_sqrt, ema_w; };

// torch.optim.Adam's arithmetic (weight_decay 0, amsgrad off): lerp_, mul_ + addcmul_, sqrt / bc2_sqrt + eps, addcdiv_
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamK& k) {
  g *= k.clip;
  m = m + (g - m) * k.omb1;
  v = k.beta2 * v + k.omb2 * g * g;
  p = p - k.step_size * (m / (sqrtf(v) / k.bc2_sqrt + k.eps));
}
__device__ __forceinline__ void ema1(float& e, float p, const AdamK& k) { e = e + k.ema_w * (p - e); }

__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(const ns2_optim_tensor* __restrict__ tensors,
                                                                   const OptChunk* __restrict__ chunks, const uint32_t* __restrict__ state,
                                                                   float omb1, float beta2, float omb2, float eps) {
  const int* iw = reinterpret_cast<const int*>(state);
  if (iw[NS2_OPTIM_W_SKIP]) return;                              // a skipped step writes nothing
  const float* f = reinterpret_cast<const float*>(state);
  const OptChunk c = chunks[blockIdx.x];
  const ns2_optim_tensor T = tensors[c.tensor];
  const bool adam = T.grad != nullptr, ema = T.ema != nullptr && iw[NS2_OPTIM_W_EMA_DUE] != 0;
  if (!adam && !ema) return;
  const AdamK k = {f[NS2_OPTIM_W_CLIP_COEF], omb1, beta2, omb2, eps, f[NS2_OPTIM_W_STEP_SIZE], f[NS2_OPTIM_W_BC2_SQRT], f[NS2_OPTIM_W_EMA_WEIGHT]};
  float* p = T.param + c.start;
  const float* g = adam ? T.grad + c.start : nullptr;
  float* m = T.exp_avg + c.start;
  float* v = T.exp_avg_sq + c.start;
  float* e = ema ? T.ema + c.start : nullptr;
  const unsigned low = low4(p);
  const bool same = (!adam || (low4(g) == low && low4(m) == low && low4(v) == low)) && (!ema || low4(e) == low);
  const int head = same ? head_of(low, c.len) : c.len;          // arrays that disagree modulo 16: the whole chunk 4 bytes at a time
  const int nv = (c.len - head) >> 2, tail0 = head + 4 * nv;
  const int t = threadIdx.x;
  for (int i = t; i < nv; i += OPT_THREADS) {
    const int o = head + 4 * i;
    float4 pp = *reinterpret_cast<const float4*>(p + o);
    if (adam) {
      const float4 gg = *reinterpret_cast<const float4*>(g + o);
      float4 mm = *reinterpret_cast<const float4*>(m + o), vv = *reinterpret_cast<const float4*>(v + o);
      adam1(pp.x, gg.x, mm.x, vv.x, k); adam1(pp.y, gg.y, mm.y, vv.y, k);
      adam1(pp.z, gg.z, mm.z, vv.z, k); adam1(pp.w, gg.w, mm.w, vv.w, k);
      *reinterpret_cast<float4*>(p + o) = pp;
      *reinterpret_cast<float4*>(m + o) = mm;
      *reinterpret_cast<float4*>(v + o) = vv;
    }
    if (ema) {
      float4 ee = *reinterpret_cast<const float4*>(e + o);
      ema1(ee.x, pp.x, k); ema1(ee.y, pp.y, k); ema1(ee.z, pp.z, k); ema1(ee.w, pp.w, k);
      *reinterpret_cast<float4*>(e + o) = ee;
    }
  }
  for (int j = t; j < head + (c.len - tail0); j += OPT_THREADS) {   // the values outside the 16-byte body
    const int o = j < head ? j : tail0 + (j - head);
    float pp = p[o];
    if (adam) {
      float mm = m[o], vv = v[o];
      adam1(pp, g[o], mm, vv, k);
      p[o] = pp; m[o] = mm; v[o] = vv;
    }
    if (ema) {
      float ee = e[o];
      ema1(ee, pp, k);
      e[o] = ee;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- small ones
struct GradPtrs { const float* p[NS2_OPTIM_GRADS_MAX]; };       // launch arguments: a captured launch keeps them by value
__global__ __launch_bounds__(NS2_OPTIM_GRADS_MAX) void optim_set_grads_kernel(ns2_optim_tensor* tensors, int first, int count, GradPtrs ptrs) {
  const int t = threadIdx.x;
  if (t < count) tensors[first + t].grad = ptrs.p[t];
}

__global__ __launch_bounds__(64) void optim_mark_kernel(uint32_t* state) {
  const int t = threadIdx.x;
  const int* iw = reinterpret_cast<const int*>(state);
  const volatile unsigned int* const* addr = reinterpret_cast<const volatile unsigned int* const*>(state + W_ADDR);
  if (t < iw[W_NCOUNTERS] && t < SAT_COUNTERS_MAX) state[W_SNAP + t] = *addr[t];
  if (t == 0) state[W_MARKED] = 1u;
}

inline bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace
}  // namespace ns2

using namespace ns2;

extern "C" int64_t ns2_optim_chunks(const ns2_optim_tensor* host_tensors, int n) {
  if (n < 0 || (n > 0 && !host_tensors)) { set_error("ns2_optim_chunks: n >= 0 tensors"); return NS2_ERR_ARG; }
  int64_t c = 0;
  for (int i = 0; i < n; ++i) {
    if (host_tensors[i].numel < 0) { set_error("ns2_optim_chunks: tensor %d has a negative numel", i); return NS2_ERR_ARG; }
    c += chunks_of(host_tensors[i].numel);
  }
  return c;
}

extern "C" int64_t ns2_optim_table_bytes(int n, int64_t chunks) {
  if (n < 0 || chunks < 0) { set_error("ns2_optim_table_bytes: n >= 0, chunks >= 0"); return NS2_ERR_ARG; }
  return off_partials(n, chunks) + chunks * (int64_t)sizeof(float);
}

extern "C" int ns2_optim_table_build(const ns2_optim_tensor* host_tensors, int n, void* table, int64_t table_bytes, void* stream) {
  const int64_t chunks = ns2_optim_chunks(host_tensors, n);
  if (chunks < 0) return NS2_ERR_ARG;
  ARGCHK(chunks < ((int64_t)1 << 31), "ns2_optim_table_build: more than 2^31 - 1 chunks");
  ARGCHK(table != nullptr && aligned16(table), "ns2_optim_table_build: the table is 16-byte aligned device memory");
  ARGCHK(table_bytes >= ns2_optim_table_bytes(n, chunks), "ns2_optim_table_build: the table is smaller than ns2_optim_table_bytes(n, ns2_optim_chunks(...))");
  std::vector<char> img((size_t)off_partials(n, chunks));
  ns2_optim_tensor* T = reinterpret_cast<ns2_optim_tensor*>(img.data());
  OptChunk* C = reinterpret_cast<OptChunk*>(img.data() + off_chunks(n));
  int64_t c = 0;
  for (int i = 0; i < n; ++i) {
    const ns2_optim_tensor& t = host_tensors[i];
    if (!(aligned4(t.param) && aligned4(t.grad) && aligned4(t.exp_avg) && aligned4(t.exp_avg_sq) && aligned4(t.ema))) {
      set_error("ns2_optim_table_build: tensor %d: every array is 4-byte aligned fp32", i);
      return NS2_ERR_ARG;
    }
    if (t.numel > 0 && !(t.param && t.exp_avg && t.exp_avg_sq)) {
      set_error("ns2_optim_table_build: tensor %d: param, exp_avg and exp_avg_sq may not be null (grad and ema may)", i);
      return NS2_ERR_ARG;
    }
    T[i] = t;
    for (int64_t s = 0; s < t.numel; s += NS2_OPTIM_CHUNK)
      C[c++] = {s, i, (int)(t.numel - s < NS2_OPTIM_CHUNK ? t.numel - s : NS2_OPTIM_CHUNK)};
  }
  if (img.empty()) return NS2_OK;
  hipStream_t s = (hipStream_t)stream;
  HIPRET(hipMemcpyAsync(table, img.data(), img.size(), hipMemcpyHostToDevice, s));
  HIPRET(hipStreamSynchronize(s));                   // the image is this call's own memory
  return NS2_OK;
}

extern "C" int ns2_optim_set_grads(void* table, int n, int first, int count, const float* const* host_grads, void* stream) {
  ARGCHK(table != nullptr && host_grads != nullptr, "ns2_optim_set_grads: null pointer");
  ARGCHK(count >= 1 && count <= NS2_OPTIM_GRADS_MAX, "ns2_optim_set_grads: 1 <= count <= NS2_OPTIM_GRADS_MAX");
  ARGCHK(first >= 0 && n >= 0 && first <= n - count, "ns2_optim_set_grads: tensors [first, first + count) of the table's n");
  GradPtrs ptrs = {};
  for (int i = 0; i < count; ++i) {
    ARGCHK(aligned4(host_grads[i]), "ns2_optim_set_grads: a grad is 4-byte aligned fp32 (or null)");
    ptrs.p[i] = host_grads[i];
  }
  hipLaunchKernelGGL(optim_set_grads_kernel, dim3(1), dim3(NS2_OPTIM_GRADS_MAX), 0, (hipStream_t)stream,
                     reinterpret_cast<ns2_optim_tensor*>(table), first, count, ptrs);
  HIPRET(hipGetLastError());
  return NS2_OK;
}

extern "C" int ns2_optim_state_init(void* state, int step, float lr, float ema_decay, void* stream) {
  ARGCHK(state != nullptr && aligned16(state), "ns2_optim_state_init: the state block is 16-byte aligned device memory");
  ARGCHK(step >= 0, "ns2_optim_state_init: step >= 0");
  int n = 0;
  const SatCounter* regs = sat_counters(&n);
  ARGCHK(regs != nullptr, "ns2_optim_state_init: more translation units registered a range counter than SAT_COUNTERS_MAX holds");
  uint32_t img[NS2_OPTIM_STATE_WORDS] = {};
  float* f = reinterpret_cast<float*>(img);
  f[NS2_OPTIM_W_CLIP_COEF] = 1.0f;
  img[NS2_OPTIM_W_STEP] = (uint32_t)step;
  f[NS2_OPTIM_W_LR] = lr;
  f[NS2_OPTIM_W_EMA_DECAY] = ema_decay;
  img[W_NCOUNTERS] = (uint32_t)n;
  for (int i = 0; i < n; ++i) {
    const uint64_t a = (uint64_t)(uintptr_t)regs[i].address();
    if (!a) {
      set_error("ns2_optim_state_init: could not take the address of range counter %d", i);
      return NS2_ERR_HIP;
    }
    img[W_ADDR + 2 * i] = (uint32_t)a;
    img[W_ADDR + 2 * i + 1] = (uint32_t)(a >> 32);
  }
  hipStream_t s = (hipStream_t)stream;
  HIPRET(hipMemcpyAsync(state, img, sizeof img, hipMemcpyHostToDevice, s));
  HIPRET(hipStreamSynchronize(s));
  return NS2_OK;
}

extern "C" int ns2_optim_mark(void* state, void* stream) {
  ARGCHK(state != nullptr && aligned16(state), "ns2_optim_mark: the state block is 16-byte aligned device memory");
  hipLaunchKernelGGL(optim_mark_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<uint32_t*>(state));
  HIPRET(hipGetLastError());
  return NS2_OK;
}

extern "C" int ns2_optim_step(void* table, int n, int64_t chunks, void* state, const ns2_optim_config* host_config, void* stream) {
  ARGCHK(host_config != nullptr, "ns2_optim_step: null config");
  const ns2_optim_config& cfg = *host_config;
  ARGCHK(n >= 0 && chunks >= 0 && chunks < ((int64_t)1 << 31), "ns2_optim_step: n >= 0, 0 <= chunks < 2^31");
  ARGCHK(state != nullptr && aligned16(state), "ns2_optim_step: the state block is 16-byte aligned device memory");
  ARGCHK(chunks == 0 || (table != nullptr && aligned16(table)), "ns2_optim_step: the table is 16-byte aligned device memory");
  ARGCHK(cfg.beta1 >= 0.0 && cfg.beta1 < 1.0 && cfg.beta2 >= 0.0 && cfg.beta2 < 1.0, "ns2_optim_step: betas in [0, 1)");
  ARGCHK(cfg.eps >= 0.0, "ns2_optim_step: eps >= 0");
  ARGCHK(cfg.max_grad_norm == cfg.max_grad_norm, "ns2_optim_step: max_grad_norm is NaN (<= 0 turns clipping off)");
  hipStream_t s = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(table);
  const ns2_optim_tensor* T = reinterpret_cast<const ns2_optim_tensor*>(base);
  const OptChunk* C = reinterpret_cast<const OptChunk*>(base + off_chunks(n));
  float* partial = reinterpret_cast<float*>(base + off_partials(n, chunks));
  uint32_t* st = reinterpret_cast<uint32_t*>(state);
  if (chunks > 0) {
    hipLaunchKernelGGL(optim_norm_kernel, dim3((unsigned)chunks), dim3(OPT_THREADS), 0, s, T, C, partial);
    HIPRET(hipGetLastError());
  }
  hipLaunchKernelGGL(optim_finish_kernel, dim3(1), dim3(FIN_THREADS), 0, s, (const float*)partial, chunks, st, cfg.beta1, cfg.beta2,
                     cfg.max_grad_norm, cfg.ema_update_every);
  HIPRET(hipGetLastError());
  if (chunks > 0) {
    hipLaunchKernelGGL(optim_update_kernel, dim3((unsigned)chunks), dim3(OPT_THREADS), 0, s, T, C, (const uint32_t*)st,
                       (float)(1.0 - cfg.beta1), (float)cfg.beta2, (float)(1.0 - cfg.beta2), (float)cfg.eps);
    HIPRET(hipGetLastError());
  }
  return NS2_OK;
}
