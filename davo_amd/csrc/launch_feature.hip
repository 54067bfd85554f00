// launch_feature.hip — the feature export kernels (feature_export.h) and their dispatch.
#include "feature_export.h"
#include "input_types.h"
#include "launch.h"

namespace davo {

hipError_t launch_feature_maps(const uint8_t* d_img, const void* d_seg, const InputFormat& fmt, const float* d_tab, const Variant& v, int nw, int H, int W,
                               float* d_att_19, float* d_attention, float* d_masked, float* d_image, hipStream_t s,
                               const void* d_depth, const float* d_tab_far, float depth_thr) {
    if (!valid(fmt)) return hipErrorInvalidValue;             // (the plain form reads no depth; a bad depth format is refused all the same)
    if (nw < 1 || H < 16 || W < 16 || H % 4 || W % 4 || !d_img || !d_seg || !d_tab) return hipErrorInvalidValue;
    if (!d_att_19 && !d_attention && !d_masked && !d_image) return hipSuccess;
    const long nthreads = (long)nw * H * (W / 4);             // >= 3 * nw * 19: the att_19 rows fit the first threads
    const FeatureMapsOut o{d_att_19, d_attention, d_masked, d_image};
    const dim3 grid((unsigned)((nthreads + 255) / 256));
    const bool split = v.att_source == ATT_DEPTH_SPLIT;       // two tables per frame: no att_19 rows (api.hip refuses the member)
    if (split && (d_att_19 || !d_depth || ((uintptr_t)d_depth & 15) || !d_tab_far)) return hipErrorInvalidValue;
    const DepthSplitArgs ds{d_depth, d_tab_far, depth_thr};
    return with_label(fmt, [&](auto L) {
        using LT = elem_t<decltype(L)>;
        if (split)
            return with_depth(fmt, [&](auto D) {
                using DT = elem_t<decltype(D)>;
                hipLaunchKernelGGL((feature_maps_depthsplit<LT, DT>), grid, dim3(256), 0, s, d_img, typed(L, d_seg), d_tab, v, nw, H, W, o, depth_split_of<DT>(ds));
                return hipGetLastError();
            });
        hipLaunchKernelGGL(feature_maps<LT>, grid, dim3(256), 0, s, d_img, typed(L, d_seg), d_tab, v, nw, H, W, o);
        return hipGetLastError();
    });
}

hipError_t launch_feature_resize_cnv6(bool h3, const void* d_cnv6, int w0, int nw, int H2, int W2, int c6, float unscale,
                                      float* d_rot, float* d_trans, hipStream_t s) {
    int cq_log2 = 0;
    while ((4 << cq_log2) < c6) ++cq_log2;
    if (nw < 1 || w0 < 0 || H2 < 1 || W2 < 1 || c6 < 32 || c6 > 256 || (4 << cq_log2) != c6 || !d_cnv6) return hipErrorInvalidValue;
    if (!d_rot && !d_trans) return hipSuccess;
    ResizeParams p{};
    p.x = static_cast<const uint8_t*>(d_cnv6);
    p.out[0] = d_rot; p.out[1] = d_trans;
    p.w0 = w0; p.nw = nw; p.H2 = H2; p.W2 = W2; p.c6 = c6; p.cq_log2 = cq_log2;
    p.head0 = d_rot ? 0 : 1;
    p.unscale = unscale;
    const long nthreads = ((long)nw * H2 * (4 * W2)) << cq_log2;
    const dim3 grid((unsigned)((nthreads + 255) / 256), (d_rot && d_trans) ? 2 : 1);
    if (h3) hipLaunchKernelGGL(feature_resize_cnv6<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(feature_resize_cnv6<false>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_feature_heat(bool h3, const void* d_cnv6, int w0, int nw, int H2, int W2, int c6, float unscale,
                               float* d_sum_rot, float* d_sum_trans, float* d_max_rot, float* d_max_trans,
                               float* d_plane_rot, float* d_plane_trans, hipStream_t s) {
    int cq_log2 = 0;
    while ((4 << cq_log2) < c6) ++cq_log2;
    if (nw < 1 || w0 < 0 || H2 < 1 || W2 < 1 || c6 < 32 || c6 > 256 || (4 << cq_log2) != c6 || !d_cnv6) return hipErrorInvalidValue;
    const bool rot = d_sum_rot && d_max_rot, trans = d_sum_trans && d_max_trans;
    if ((d_plane_rot && !rot) || (d_plane_trans && !trans)) return hipErrorInvalidValue;
    if (!rot && !trans) return hipSuccess;
    HeatParams p{};
    p.x = static_cast<const uint8_t*>(d_cnv6);
    p.sum[0] = rot ? d_sum_rot : nullptr; p.sum[1] = trans ? d_sum_trans : nullptr;
    p.max[0] = rot ? reinterpret_cast<unsigned*>(d_max_rot) : nullptr; p.max[1] = trans ? reinterpret_cast<unsigned*>(d_max_trans) : nullptr;
    p.w0 = w0; p.nw = nw; p.H2 = H2; p.W2 = W2; p.c6 = c6; p.cq_log2 = cq_log2;
    p.head0 = rot ? 0 : 1;
    p.unscale = unscale;
    for (int h = 0; h < 2; ++h)
        if (p.max[h]) { hipError_t e = hipMemsetAsync(p.max[h], 0, (size_t)nw * sizeof(unsigned), s); if (e != hipSuccess) return e; }
    const long npix = (long)nw * H2 * W2;
    const dim3 grid((unsigned)(((npix << cq_log2) + 255) / 256), (rot && trans) ? 2 : 1);
    if (h3) hipLaunchKernelGGL(feature_heat_cnv6<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(feature_heat_cnv6<false>, grid, dim3(256), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || (!d_plane_rot && !d_plane_trans)) return e;
    PlaneParams q{};
    q.sum[0] = d_sum_rot; q.sum[1] = d_sum_trans;
    q.out[0] = d_plane_rot; q.out[1] = d_plane_trans;
    q.nw = nw; q.H2 = H2; q.W2 = W2;
    q.head0 = d_plane_rot ? 0 : 1;
    hipLaunchKernelGGL(feature_resize_plane, dim3((unsigned)((npix + 255) / 256), (d_plane_rot && d_plane_trans) ? 2 : 1), dim3(256), 0, s, q);
    return hipGetLastError();
}

}  // namespace davo
