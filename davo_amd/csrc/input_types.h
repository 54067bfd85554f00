// input_types.h — the one place that turns an InputFormat (params.h) into element types.  Host side, for the launch units: a
// helper per plane kind calls a generic callable with a tag of the plane's element type and returns what the callable returns;
// a format value that names no element type is hipErrorInvalidValue and the callable is not called.  A launcher nests the
// helpers of exactly the plane kinds its kernel is templated on, so the instantiated kernels are the cross product written - and
// they land in the code object in the order the nest visits them (a helper tries the narrow type first), which the launchers
// keep as it has always been: the same kernels at the same addresses (profiles/input_format_code_objects.md):
//   return with_flow(fmt, [&](auto F) { return with_label(fmt, [&](auto L) {
//       hipLaunchKernelGGL((kernel<elem_t<decltype(L)>, elem_t<decltype(F)>>), ...);
//       return hipGetLastError();
//   }); });
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "input_decode.h"
#include "params.h"

namespace davo {

template <typename T> struct ElemTag { using type = T; };
template <typename Tag> using elem_t = typename Tag::type;

// labels: float | uint8_t
template <typename Fn>
__attribute__((always_inline)) inline hipError_t with_label(const InputFormat& f, Fn&& fn) {
    if (f.label == LABELS_U8) return fn(ElemTag<uint8_t>{});
    if (f.label == LABELS_F32) return fn(ElemTag<float>{});
    return hipErrorInvalidValue;
}
// flow: float | in_f16
template <typename Fn>
__attribute__((always_inline)) inline hipError_t with_flow(const InputFormat& f, Fn&& fn) {
    if (f.flow == FLOW_F16) return fn(ElemTag<in_f16>{});
    if (f.flow == FLOW_F32) return fn(ElemTag<float>{});
    return hipErrorInvalidValue;
}
// depth: float | in_f16
template <typename Fn>
__attribute__((always_inline)) inline hipError_t with_depth(const InputFormat& f, Fn&& fn) {
    if (f.depth == DEPTH_F16) return fn(ElemTag<in_f16>{});
    if (f.depth == DEPTH_F32) return fn(ElemTag<float>{});
    return hipErrorInvalidValue;
}

// a raw input pointer as the element type a tag names
template <typename Tag>
inline const elem_t<Tag>* typed(Tag, const void* p) { return static_cast<const elem_t<Tag>*>(p); }

// the depth-split arguments as the host hands them on (the planes in the context's depth format); typed where the kernel is chosen
struct DepthSplitArgs { const void* depth; const float* tab_far; float thr; };
template <typename DT>
DepthSplitOf<DT> depth_split_of(const DepthSplitArgs& a) { return DepthSplitOf<DT>{static_cast<const DT*>(a.depth), a.tab_far, a.thr}; }

}  // namespace davo
