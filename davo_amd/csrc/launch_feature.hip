// launch_feature.hip — the feature export kernels (feature_export.h) and their dispatch.
#include "feature_export.h"
#include "launch.h"

namespace davo {

hipError_t launch_feature_maps(const uint8_t* d_img, const float* d_seg, const float* d_tab, const Variant& v, int nw, int H, int W,
                               float* d_att_19, float* d_attention, float* d_masked, float* d_image, hipStream_t s) {
    if (nw < 1 || H < 16 || W < 16 || H % 4 || W % 4 || !d_img || !d_seg || !d_tab) return hipErrorInvalidValue;
    if (!d_att_19 && !d_attention && !d_masked && !d_image) return hipSuccess;
    const long nthreads = (long)nw * H * (W / 4);             // >= 3 * nw * 19: the att_19 rows fit the first threads
    const FeatureMapsOut o{d_att_19, d_attention, d_masked, d_image};
    hipLaunchKernelGGL(feature_maps, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, s, d_img, d_seg, d_tab, v, nw, H, W, o);
    return hipGetLastError();
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

}  // namespace davo
