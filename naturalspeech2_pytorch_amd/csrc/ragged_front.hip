// Ragged prompts and text (include/ns2hip_frontend.h): what the front-end needs, beside the attention kernels' key counts and key
// masks, so that utterance i of a padded batch equals utterance i alone with its text cut to text_lens[i] and its prompt to prompt_lens[i]:
//   - GroupNorm + SiLU with a row count per utterance (the <true> kernels of groupnorm_kernel.h);
//   - zero-filling the rows behind a length, for the "same" convolutions that would otherwise read their neighbours' padding;
//   - the mean over the valid prompt rows (Model's to_prompt_cond) and the key counts Lm + len of the perceiver resampler.
// Lengths are int32 [B] in device memory, read here alone and clamped into [1, n].  The GEMM and attention kernels are not touched: row
// masking is a launch of its own.  ns2_model_prepare_cond_lens, the fourth entry of the header, lives with the executor (model_exec.cpp).
#include <hip/hip_runtime.h>

#include "../../include/ns2hip_frontend.h"
#include "groupnorm_kernel.h"

namespace ns2 {

NS2_DEVINL int clamp_len(const int* lens, int b, int n) { return min(max(lens[b], 1), n); }

// ---------------------------------------------------------------- zero rows
constexpr int ZR_THREADS = 256;
constexpr int ZR_ROWS = 8;

// grid (ceil(n / ZR_ROWS), B); q = 16-byte vectors per row.  A block wholly before the length writes nothing.
__global__ __launch_bounds__(ZR_THREADS) void zero_rows_kernel(uint4* buf, long q, int n, const int* lens) {
  const int b = blockIdx.y, r0 = blockIdx.x * ZR_ROWS;
  const int len = clamp_len(lens, b, n);
  const int r1 = min(r0 + ZR_ROWS, n);
  const int rs = max(r0, len);                          // first row of this block to clear
  if (rs >= r1) return;
  uint4* base = buf + ((long)b * n + rs) * q;           // rows rs .. r1 - 1 are contiguous
  const long total = (long)(r1 - rs) * q;
  for (long i = threadIdx.x; i < total; i += ZR_THREADS) base[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---------------------------------------------------------------- masked mean over rows, key counts of cat(latents, prompt)
// the loop of mean_rows_kernel (elementwise.hip) stopped at the utterance's length: ascending rows, one thread per column
__global__ void mean_rows_lens_kernel(const float* in, int n, int d, const int* lens, float* out) {
  const int b = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d) return;
  const int len = clamp_len(lens, b, n);
  float acc = 0.f;
  for (int i = 0; i < len; ++i) acc += in[((long)b * n + i) * d + c];
  out[(long)b * d + c] = acc / (float)len;
}

__global__ void offset_lens_kernel(const int* lens, int B, int n, int offset, int* out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) out[b] = offset + clamp_len(lens, b, n);
}

hipError_t launch_mean_rows_lens(const float* in, int B, int n, int d, const int* lens, float* out, hipStream_t s) {
  if (!in || !lens || !out || B <= 0 || B > 65535 || n <= 0 || d <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mean_rows_lens_kernel, dim3((d + 255) / 256, B), dim3(256), 0, s, in, n, d, lens, out);
  return hipGetLastError();
}

// out[b] = offset + clamp(lens[b], 1, n): the keys utterance b attends to in cat(offset latents, n prompt rows)
hipError_t launch_offset_lens(const int* lens, int B, int n, int offset, int* out, hipStream_t s) {
  if (!lens || !out || B <= 0 || n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(offset_lens_kernel, dim3((B + 255) / 256), dim3(256), 0, s, lens, B, n, offset, out);
  return hipGetLastError();
}

}  // namespace ns2

using namespace ns2;

#define RF_HIPRET(expr)                                                              \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return NS2_ERR_HIP;                                                            \
    }                                                                                \
  } while (0)

extern "C" int ns2_groupnorm_silu_lens(const float* x, int B, int n, int C, int groups, const float* weight, const float* bias, float eps,
                                       const float* resid, const int* row_lens, float* out_f32, uint16_t* out_hi, uint16_t* out_lo,
                                       int ldo, int precision, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!row_lens)
    return ns2_groupnorm_silu(x, B, n, C, groups, weight, bias, eps, resid, out_f32, out_hi, out_lo, ldo, precision, workspace,
                              workspace_bytes, stream);
  GnArgs a;
  const int rc = gn_fill_args("ns2_groupnorm_silu_lens", x, B, n, C, groups, weight, bias, eps, resid, out_f32, out_hi, out_lo, ldo,
                              precision, workspace, workspace_bytes, &a);
  if (rc != NS2_OK) return rc;
  ARGCHK(B <= 65535, "ns2_groupnorm_silu_lens: at most 65535 utterances");
  a.row_lens = row_lens;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gn_stats_kernel<true>, dim3(a.nchunks, groups, B), dim3(GN_THREADS), 0, s, a);
  RF_HIPRET(hipGetLastError());
  hipLaunchKernelGGL(gn_apply_kernel<true>, dim3((n + GN_APPLY_ROWS - 1) / GN_APPLY_ROWS, B), dim3(GN_THREADS), 3 * groups * sizeof(float),
                     s, a);
  RF_HIPRET(hipGetLastError());
  return NS2_OK;
}

extern "C" int ns2_zero_rows_lens(void* buf, int64_t row_bytes, int B, int n, const int* lens, void* stream) {
  ARGCHK(buf && lens && B > 0 && n > 0 && row_bytes > 0, "ns2_zero_rows_lens: bad arguments");
  ARGCHK(B <= 65535, "ns2_zero_rows_lens: at most 65535 utterances");
  ARGCHK(row_bytes % 16 == 0 && (uintptr_t)buf % 16 == 0, "ns2_zero_rows_lens: rows are whole 16-byte vectors of a 16-byte aligned buffer");
  hipLaunchKernelGGL(zero_rows_kernel, dim3((n + ZR_ROWS - 1) / ZR_ROWS, B), dim3(ZR_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<uint4*>(buf), (long)(row_bytes / 16), n, lens);
  RF_HIPRET(hipGetLastError());
  return NS2_OK;
}

extern "C" int ns2_mean_rows_lens(const float* in, int B, int n, int d, const int* lens, float* out, void* stream) {
  ARGCHK(in && lens && out && B > 0 && n > 0 && d > 0, "ns2_mean_rows_lens: bad arguments");
  ARGCHK(B <= 65535, "ns2_mean_rows_lens: at most 65535 utterances");
  RF_HIPRET(launch_mean_rows_lens(in, B, n, d, lens, out, (hipStream_t)stream));
  return NS2_OK;
}
