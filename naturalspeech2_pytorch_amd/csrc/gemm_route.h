// Host-only interface between gemm.hip and gemm2.hip: which kernel launch_gemm runs a product on, and the launchers of the
// 128 x 128 kernel that gemm2.hip's dispatch calls.  Not part of the library's interface (ns2_kernels.h).
#pragma once
#include "ns2_kernels.h"

namespace ns2 {

// SplitK: K slices on the 128 x 128 kernel + the finishing launch (gemm.hip); Tile128 / Tile256: one launch of the 128 x 128
// kernel (gemm.hip) / of the 256 x 256 kernel (gemm2.hip); FfConv3 / Linear3 / Wavenet3: the dedicated kernels of
// ffconv_kernel.h / gemm3_kernel.h / wavenet3_kernel.h
enum class GemmRoute { SplitK, Tile128, Tile256, FfConv3, Linear3, Wavenet3 };
struct GemmPlan {
  GemmRoute route;
  int S, c;          // SplitK: S slices of c K tiles of every tap (splitk_plan); any other route: S = 1, c = kt_per_tap
};

// The kernel launch_gemm runs g on, under the test hook's current mode (force_gemm_kernel).  Pure host arithmetic: no HIP call.
GemmPlan plan_gemm(const GemmArgs& g, int precision);
// test hook (ns2_debug_gemm_route_launches): products launch_gemm has sent down `route` (the enum's order, 0 = SplitK ... 5 = Wavenet3) so far
long long gemm_route_launches(int route);

// gemm.hip.  g: validated by launch_gemm, formats resolved.
hipError_t launch_gemm1(const GemmArgs& g, int precision, hipStream_t s);                      // the 128 x 128 register-staged kernel
hipError_t launch_gemm_splitk(const GemmArgs& g, int precision, int S, int c, hipStream_t s);  // K slices into g.sk_ws + the finishing launch

}  // namespace ns2
