// Host-side launch helpers shared by every extern "C" entry: the width sets the kernels are instantiated for and the one
// dispatch over them, and the opt-in to more than 64 KB of dynamic LDS.
#pragma once
#include "mgv_common.h"
#include <atomic>
#include <type_traits>

namespace mgv {

// ---------------------------------------------------------------------------------- width dispatch
template <int... W> struct Widths {};

using AllWidths  = Widths<16, 32, 64, 128>;   // float4-per-lane gather / reduction kernels
using LaneWidths = Widths<16, 32, 64>;        // one float per lane (a row must fit a wave) and the exact-fp32 stage / level kernels
using X3Widths   = Widths<32, 64>;            // bf16x3 stage / level kernels
using PoolWidths = Widths<32, 64, 128>;       // attention pool

template <int W> using Width = std::integral_constant<int, W>;

template <int... W>
constexpr bool has_width(Widths<W...>, int H) { return ((H == W) || ...); }

// f(Width<W>{}) for the W that equals H, and its result; MGV_EUNSUPPORTED (f never called) when H is not in the set
template <int... W, typename F>
inline int dispatch_width(Widths<W...>, int H, F&& f) {
    int rc = MGV_EUNSUPPORTED;
    (void)((H == W && ((rc = f(Width<W>{})), true)) || ...);
    return rc;
}

// the common case: f only launches, and the entry returns what the launches left behind
template <int... W, typename F>
inline int launch_width(Widths<W...> set, int H, F&& f) {
    return dispatch_width(set, H, [&](auto w) { f(w); MGV_LAUNCH_RET(); });
}

// ---------------------------------------------------------------------------------- dynamic LDS above the default limit
// A kernel that asks for more than 64 KB of dynamic LDS must be allowed to, once per DEVICE: each device loads its own copy of the
// code object, and the attribute belongs to that copy.  One memo per (kernel, bytes) and device; a launch costs one hipGetDevice.
constexpr int kMaxDevices = 64;

template <auto Kernel, int Bytes = 160 * 1024>
inline void allow_lds() {
    static std::atomic<bool> set[kMaxDevices] = {};
    int dev = 0;
    const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kMaxDevices;
    if (known && set[dev].load(std::memory_order_relaxed)) return;
    hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, Bytes);
    if (known) set[dev].store(true, std::memory_order_relaxed);
}

}  // namespace mgv
