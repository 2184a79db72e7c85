// Registry of the range-guard counters (ns2_common.h): every translation unit that includes ns2_common.h owns one
// `static __device__` counter and hands its host-side readers to register_sat_counter() while the library is loaded.
// capi.cpp keeps the registry and loops over it (ns2_saturation_count / _counters / _counter_name / _peek).
#pragma once
#include <hip/hip_runtime.h>

namespace ns2 {

struct SatCounter {
  unsigned int (*read)(bool reset);                      // synchronising read (~0u: the read failed), optionally zeroing the counter
  hipError_t (*peek)(unsigned int* dst, hipStream_t s);  // stream-ordered, non-synchronising copy into (pinned) host memory
  void* (*address)();                                    // the counter's address on the current device (null: the lookup failed), for
                                                         // kernels that read it in stream order (optim.hip: mark / skip)
  const char* file;                                      // __BASE_FILE__ of the translation unit
};

constexpr int SAT_COUNTERS_MAX = 32;
// called from static initialisers: no allocation, no HIP call.  One registration too many is remembered and every reader fails on it.
void register_sat_counter(const SatCounter& c);
// the registered counters (count in *n); nullptr when more than SAT_COUNTERS_MAX tried to register
const SatCounter* sat_counters(int* n);

}  // namespace ns2
