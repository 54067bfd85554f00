// launch_misc.hip — the small kernels of the path (SE squeeze/excite, mask + pack, pose head, the
// cnv1 LDS-patch kernel, the direct-convolution cross-check) and the per-device attribute cache.
#include <algorithm>
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>

#include "conv_patch_h3.h"
#include "conv_patch_f32.h"
#include "input_types.h"
#include "launch.h"
#include "owned.h"
#include "posenn_se.h"
#include "prologue.h"
#include "se_pool.h"
#include "window_gather.h"
#include "window_mirror.h"

namespace davo {

hipError_t ensure_dynamic_lds(const void* kernel, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_pair(dev, kernel);
    if (done.count(key)) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.insert(key);
    return e;
}

namespace {
// a run-time choice among a kernel's non-type template arguments, as a constant the callable can name (input_types.h does the
// same for the element types)
template <typename Fn>
__attribute__((always_inline)) inline hipError_t with_bool(bool b, Fn&& fn) {
    return b ? fn(std::true_type{}) : fn(std::false_type{});
}
template <typename Fn>
__attribute__((always_inline)) inline hipError_t with_pack_ld(int ld, Fn&& fn) {
    if (ld == 16) return fn(std::integral_constant<int, 16>{});
    if (ld == 8) return fn(std::integral_constant<int, 8>{});
    if (ld == 10) return fn(std::integral_constant<int, 10>{});
    return hipErrorInvalidValue;
}
}  // namespace

// fmt (here and below): the context's input format (params.h) - what d_flow, d_seg and d_depth point at; a value that names no
// element type of a plane kind the kernel reads is an error
hipError_t launch_se_squeeze(const void* d_flow, const InputFormat& fmt, int B, int HW, const Variant& v, float* d_partial, int sel, hipStream_t s) {
    const dim3 grid(SQ_CHUNKS, pairs_per_window(sel), B);
    return with_flow(fmt, [&](auto F) {
        hipLaunchKernelGGL(se_squeeze_partial<elem_t<decltype(F)>>, grid, dim3(256), 0, s, typed(F, d_flow), HW, v.norm_flow, v.abs_mode, sel, d_partial);
        return hipGetLastError();
    });
}

hipError_t launch_se_excite(const float* d_partial, int B, int HW, const Variant& v, const SeDense& w, const float* wstatic, float* d_tab,
                            unsigned* d_range_reset, int sel, hipStream_t s) {
    hipLaunchKernelGGL(se_excite, dim3(B, 3), dim3(64), 0, s, d_partial, HW, v, w.w1, w.b1, w.w2, w.b2, wstatic, d_tab, d_range_reset, sel);
    return hipGetLastError();
}

hipError_t launch_se_squeeze_excite(const void* d_flow, const InputFormat& fmt, int B, int HW, const Variant& v, float* d_partial, unsigned* d_counters,
                                    const SeDense& w, const float* wstatic, float* d_tab, unsigned* d_range_reset, int sel, hipStream_t s) {
    const dim3 grid(SQ_CHUNKS, pairs_per_window(sel), B);
    return with_flow(fmt, [&](auto F) {
        hipLaunchKernelGGL(se_squeeze_excite<elem_t<decltype(F)>>, grid, dim3(256), 0, s, typed(F, d_flow), HW, v, d_partial, d_counters, w.w1, w.b1, w.w2, w.b2,
                           wstatic, d_tab, d_range_reset, sel);
        return hipGetLastError();
    });
}

hipError_t launch_se_squeeze_excite_split(const void* d_flow, const InputFormat& fmt, int B, int HW, const Variant& v, float* d_partial, unsigned* d_counters,
                                          const SeDense& near, const SeDense& far_w, float* d_tab, float* d_tab_far,
                                          unsigned* d_range_reset, int sel, hipStream_t s) {
    if (v.att_source != ATT_DEPTH_SPLIT || !d_tab_far || !near || !far_w) return hipErrorInvalidValue;
    const SeFar far{far_w.w1, far_w.b1, far_w.w2, far_w.b2, d_tab_far};
    const dim3 grid(SQ_CHUNKS, pairs_per_window(sel), B);
    return with_flow(fmt, [&](auto F) {
        hipLaunchKernelGGL(se_squeeze_excite_split<elem_t<decltype(F)>>, grid, dim3(256), 0, s, typed(F, d_flow), HW, v, d_partial, d_counters,
                           near.w1, near.b1, near.w2, near.b2, d_tab, d_range_reset, sel, far);
        return hipGetLastError();
    });
}

hipError_t launch_se_class_squeeze(bool fold, const uint8_t* d_img, const void* d_flow, const void* d_seg, const InputFormat& fmt, int B, int H, int W,
                                  const Variant& v, unsigned* d_partial, unsigned* d_counters, const SeDense& w, float* d_tab,
                                  unsigned* d_range_reset, int sel, hipStream_t s) {
    const dim3 grid(SQ_CHUNKS, att_se_frames(v.att_source) - (sel == PAIRS_BOTH ? 0 : 1), B);
    return with_flow(fmt, [&](auto F) { return with_label(fmt, [&](auto L) { return with_bool(fold, [&](auto FOLD) {
        hipLaunchKernelGGL((se_class_squeeze<decltype(FOLD)::value, elem_t<decltype(L)>, elem_t<decltype(F)>>), grid, dim3(256), 0, s, d_img,
                           typed(F, d_flow), typed(L, d_seg), H, W, v, d_partial, d_counters, w.w1, w.b1, w.w2, w.b2, d_tab, d_range_reset, sel);
        return hipGetLastError();
    }); }); });
}

hipError_t launch_se_depth_squeeze(bool fold, const void* d_depth, const InputFormat& fmt, int B, int HW, const Variant& v, unsigned* d_partial,
                                   unsigned* d_counters, const SeDense& w, float* d_tab, unsigned* d_range_reset, int sel, hipStream_t s) {
    if (!att_desc_depth(v.att_source) || !d_depth || ((uintptr_t)d_depth & 15) || HW % 16) return hipErrorInvalidValue;
    const dim3 grid(SQ_CHUNKS, 1 + pairs_per_window(sel), B);
    return with_depth(fmt, [&](auto D) { return with_bool(fold, [&](auto FOLD) {
        hipLaunchKernelGGL((se_depth_squeeze<decltype(FOLD)::value, elem_t<decltype(D)>>), grid, dim3(256), 0, s, typed(D, d_depth), HW, v, d_partial,
                           d_counters, w.w1, w.b1, w.w2, w.b2, d_tab, d_range_reset, sel);
        return hipGetLastError();
    }); });
}

hipError_t launch_se_pool_squeeze(const void* d_flow, const InputFormat& fmt, int B, int H, int W, const Variant& v, const PoolDev& pd, float* d_partial,
                                  int sel, hipStream_t s) {
    if (!att_pooled(v.att_source) || W % 4 || pd.n_items < 1 || !pd.items || !d_flow || !d_partial) return hipErrorInvalidValue;
    const dim3 grid(pd.n_items, pairs_per_window(sel), B);
    return with_flow(fmt, [&](auto F) {
        hipLaunchKernelGGL(se_pool_squeeze<elem_t<decltype(F)>>, grid, dim3(256), 0, s, typed(F, d_flow), H, W, v, sel, pd, d_partial);
        return hipGetLastError();
    });
}

hipError_t launch_se_pool_excite(const float* d_partial, int B, const Variant& v, const PoolDev& pd, const SeDense& w, float* d_tab, float* d_desc,
                                 unsigned* d_range_reset, int sel, hipStream_t s) {
    const int a = v.att_source;
    if (!att_pooled(a) || 2 * pd.n_cells != att_se_in(a) || 2 * pd.n_cells > POOL_MAX_D || !pd.cell_first || !pd.inv_div || !d_partial || !w || !d_tab || !d_desc)
        return hipErrorInvalidValue;
    if (att_se_hidden(a) == NCLS)
        hipLaunchKernelGGL(se_pool_excite<NCLS>, dim3(B, 3), dim3(64), 0, s, d_partial, pd, v, w.w1, w.b1, w.w2, w.b2, d_tab, d_desc, d_range_reset, sel);
    else
        hipLaunchKernelGGL(se_pool_excite<8>, dim3(B, 3), dim3(64), 0, s, d_partial, pd, v, w.w1, w.b1, w.w2, w.b2, d_tab, d_desc, d_range_reset, sel);
    return hipGetLastError();
}

hipError_t launch_mask_pack(int ld, const uint8_t* d_img, const void* d_flow, const void* d_seg, const InputFormat& fmt, const float* d_tab,
                            const Variant& v, int B, int H, int W, float* d_packed, int sel, hipStream_t s,
                            const void* d_depth, const float* d_tab_far, float depth_thr) {
    const long nthreads = (long)pairs_per_window(sel) * B * H * (W / 4);
    const dim3 grid((unsigned)((nthreads + 255) / 256));
    const bool split = v.att_source == ATT_DEPTH_SPLIT;
    // the depth-split form: a missing plane or table is an error, never the plain packer
    if (split && (!d_depth || ((uintptr_t)d_depth & 15) || !d_tab_far)) return hipErrorInvalidValue;
    if (!valid(fmt)) return hipErrorInvalidValue;      // (the plain packer reads no depth; a bad depth format is refused all the same)
    const DepthSplitArgs ds{d_depth, d_tab_far, depth_thr};
    return with_flow(fmt, [&](auto F) { return with_label(fmt, [&](auto L) {
        using LT = elem_t<decltype(L)>;
        using FT = elem_t<decltype(F)>;
        if (split)
            return with_depth(fmt, [&](auto D) { return with_pack_ld(ld, [&](auto LD) {
                using DT = elem_t<decltype(D)>;
                hipLaunchKernelGGL((mask_pack_depthsplit<decltype(LD)::value, LT, FT, DT>), grid, dim3(256), 0, s, d_img, typed(F, d_flow), typed(L, d_seg), d_tab,
                                   v, B, sel, H, W, d_packed, depth_split_of<DT>(ds));
                return hipGetLastError();
            }); });
        return with_pack_ld(ld, [&](auto LD) {
            hipLaunchKernelGGL((mask_pack<decltype(LD)::value, LT, FT>), grid, dim3(256), 0, s, d_img, typed(F, d_flow), typed(L, d_seg), d_tab, v, B, sel, H, W,
                               d_packed);
            return hipGetLastError();
        });
    }); });
}

hipError_t launch_mask_pack3(bool h3, const uint8_t* d_img, const void* d_flow, const void* d_seg, const InputFormat& fmt, const float* d_tab,
                             const Variant& v, int B, int H, int W, float* d_packed, hipStream_t s) {
    if (B < 1 || H < 1 || W < 4 || W % 4 || !d_img || !d_flow || !d_seg || !d_tab || !d_packed) return hipErrorInvalidValue;
    if (att_reads_depth(v.att_source)) return hipErrorInvalidValue;      // no three-frame form of the depth sources
    const long nthreads = (long)B * H * (W / 4);
    const dim3 grid((unsigned)((nthreads + PACK3_THREADS - 1) / PACK3_THREADS));
    return with_flow(fmt, [&](auto F) { return with_label(fmt, [&](auto L) { return with_bool(h3, [&](auto H3) {
        hipLaunchKernelGGL((mask_pack3<decltype(H3)::value, elem_t<decltype(L)>, elem_t<decltype(F)>>), grid, dim3(PACK3_THREADS), 0, s, d_img,
                           typed(F, d_flow), typed(L, d_seg), d_tab, v, B, H, W, d_packed);
        return hipGetLastError();
    }); }); });
}

hipError_t launch_window_gather(const GatherArgs& a, int N, const InputFormat& fmt, hipStream_t s) {
    if (N < 1 || a.H < 1 || a.W < 4 || a.W % 4 || ((size_t)a.H * a.W) % 16 || !a.f_img || !a.f_seg || !a.w_img || !a.w_seg || !a.w_flow ||
        (a.f_depth && !a.w_depth))
        return hipErrorInvalidValue;
    if (((uintptr_t)a.f_img | (uintptr_t)a.f_seg | (uintptr_t)a.f_depth | (uintptr_t)a.f_flow | (uintptr_t)a.w_img | (uintptr_t)a.w_seg |
         (uintptr_t)a.w_depth | (uintptr_t)a.w_flow) & 15)
        return hipErrorInvalidValue;
    // the largest job decides the pieces per job (a flow plane, else a frame or a float32 plane); at most 8, the rest in rounds
    const size_t HW = (size_t)a.H * a.W;
    // (a binary16 flow plane is HW / 4 vectors, no more than a float32 label or depth plane, a binary16 depth plane HW / 8: the max below covers them)
    const size_t vecs = a.f_flow ? HW * 2 * element_bytes(fmt).flow / 16 : (a.W % 16 == 0 ? HW * 3 / 16 : HW * 3 / 4);
    const unsigned gx = (unsigned)std::min<size_t>(8, (std::max(vecs, HW / 4) + GATHER_PIECE - 1) / GATHER_PIECE);
    const dim3 grid(gx, (unsigned)N, GATHER_JOBS);
    return with_flow(fmt, [&](auto F) { return with_label(fmt, [&](auto L) { return with_depth(fmt, [&](auto D) {
        hipLaunchKernelGGL((window_gather<elem_t<decltype(L)>, elem_t<decltype(F)>, elem_t<decltype(D)>>), grid, dim3(256), 0, s, a);
        return hipGetLastError();
    }); }); });
}

hipError_t launch_window_mirror(const GatherArgs& a, int N, bool frames, const InputFormat& fmt, hipStream_t s) {
    if (N < 1 || a.H < 1 || a.W < 4 || a.W % 4 || ((size_t)a.H * a.W) % 16 || !a.f_img || !a.f_seg || !a.w_img || !a.w_seg || !a.w_flow ||
        (a.f_depth && !a.w_depth) || (!frames && !a.f_flow))
        return hipErrorInvalidValue;
    if (((uintptr_t)a.f_img | (uintptr_t)a.f_seg | (uintptr_t)a.f_depth | (uintptr_t)a.f_flow | (uintptr_t)a.w_img | (uintptr_t)a.w_seg |
         (uintptr_t)a.w_depth | (uintptr_t)a.w_flow) & 15)
        return hipErrorInvalidValue;
    // the job with the most unit pairs decides the pieces per job: a flow plane (four pixels a unit, half as many pairs a row); at
    // most 8, the rest in rounds
    const size_t pairs = (size_t)a.H * ((a.W / 4 + 1) / 2);
    const unsigned gx = (unsigned)std::min<size_t>(8, (pairs + MIRROR_PIECE - 1) / MIRROR_PIECE);
    const dim3 grid(gx, (unsigned)N, GATHER_JOBS);
    return with_depth(fmt, [&](auto D) { return with_bool(frames, [&](auto FR) { return with_flow(fmt, [&](auto F) { return with_label(fmt, [&](auto L) {
        hipLaunchKernelGGL((window_mirror<elem_t<decltype(L)>, elem_t<decltype(F)>, elem_t<decltype(D)>, decltype(FR)::value>), grid, dim3(256), 0, s, a);
        return hipGetLastError();
    }); }); }); });
}

hipError_t launch_patch_layer(int layer, bool f32, bool fused, bool cnv1t, const ConvPatchParams& p, int nblk, hipStream_t s, const InputFormat& fmt) {
    using Kernel = void (*)(ConvPatchParams);
    struct Row { Kernel h3, f32; int threads, lds; };
    if (cnv1t) {
        if (layer != 0 || f32 || fused || nblk < 1 || !p.x || !p.w || !p.bias || !p.y || !p.zeros || p.ntiles < 1) return hipErrorInvalidValue;
        const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(conv_patch_cnv1t_h3), cp1t::LDS_BYTES);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(conv_patch_cnv1t_h3, dim3(nblk), dim3(cp1::THREADS), cp1t::LDS_BYTES, s, p);
        return hipGetLastError();
    }
    // the fused cnv1 of the context's label and flow elements (p.seg and p.flow are in those formats)
    Kernel cnv1_fused = nullptr;
    const hipError_t fe = with_flow(fmt, [&](auto F) { return with_label(fmt, [&](auto L) {
        cnv1_fused = conv_patch_cnv1_h3<true, elem_t<decltype(L)>, elem_t<decltype(F)>>;
        return hipSuccess;
    }); });
    if (fe != hipSuccess) return fe;
    static const Row rows[3] = {{conv_patch_cnv1_h3<false>, conv_patch_cnv1_f32, cp1::THREADS, cp1::LDS_BYTES},
                                {conv_patch_cnv2_h3, conv_patch_cnv2_f32, cp2::THREADS, cp2::LDS_BYTES},
                                {conv_patch_cnv3_h3, conv_patch_cnv3_f32, cp3::THREADS, cp3::LDS_BYTES}};
    if (layer < 0 || layer > 2 || (fused && (f32 || layer != 0))) return hipErrorInvalidValue;
    const Row& r = rows[layer];
    const Kernel k = fused ? cnv1_fused : (f32 ? r.f32 : r.h3);
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(k), r.lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(nblk), dim3(r.threads), r.lds, s, p);
    return hipGetLastError();
}

// every workgroup records the XCD it runs on (HW_REG_XCC_ID)
__global__ __launch_bounds__(64) void xcd_probe_kernel(unsigned* out) {
    if (threadIdx.x == 0) out[blockIdx.y * gridDim.x + blockIdx.x] = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 15u;
}

hipError_t xcd_round_robin_probe(hipStream_t s, int* ok) {
    constexpr int NX = 64, NY = 4;
    DevMem<unsigned> d;
    unsigned h[NX * NY];
    *ok = 0;
    hipError_t e = dev_alloc(&d, NX * NY);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(xcd_probe_kernel, dim3(NX, NY), dim3(64), 0, s, d.get());
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h, d.get(), sizeof h, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    bool same = true;
    for (int y = 1; y < NY; ++y)
        for (int x = 0; x < NX; ++x) same = same && h[y * NX + x] == h[x];
    *ok = same ? 1 : 0;
    return hipSuccess;
}

hipError_t launch_splitk_fixup(const float* d_part, long M, int N, int S, int relu, uint8_t* d_y, unsigned* d_range, hipStream_t s) {
    if (N < 32 || N % 32 || S < 2 || M < 1) return hipErrorInvalidValue;
    const long pairs = M * (N / 2);
    hipLaunchKernelGGL(splitk_fixup, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, d_part, pairs, N, S, relu, d_y, d_range);
    return hipGetLastError();
}

hipError_t launch_pose_from_tiles(const float* d_tiles, int NB, int P, int bm, int mtiles, int ntiles_n,
                                  const float* d_bpred, float* d_pose, const SnapArgs& snap, int sel, hipStream_t s) {
    hipLaunchKernelGGL(pose_from_tiles, dim3(NB * 6), dim3(64), 0, s, d_tiles, NB, P, bm, mtiles, ntiles_n, d_bpred, d_pose, sel, snap);
    return hipGetLastError();
}

hipError_t launch_range_guard_snapshot(const SnapArgs& snap, hipStream_t s) {
    hipLaunchKernelGGL(range_guard_snapshot, dim3(256), dim3(256), 0, s, snap);
    return hipGetLastError();
}

hipError_t launch_pose_head(int cols, int heads, const float* d_c7, int NB, int P, const float* d_wpred, const float* d_bpred,
                            float* d_partial, float* d_pose, int sel, hipStream_t s) {
    if (NB < 1 || P < 1 || !d_c7 || !d_wpred || !d_bpred || !d_partial || !d_pose) return hipErrorInvalidValue;
    const dim3 grid(PH_SPLIT, NB, heads);
    if (cols == 3 && heads == 2) hipLaunchKernelGGL(pose_head_partial<3>, grid, dim3(256), 0, s, d_c7, P, d_wpred, d_partial);
    else if (cols == 6 && heads == 2) hipLaunchKernelGGL(pose_head_partial<6>, grid, dim3(256), 0, s, d_c7, P, d_wpred, d_partial);
    else if (cols == 6 && heads == 1) hipLaunchKernelGGL((pose_head_partial<6, 1>), grid, dim3(256), 0, s, d_c7, P, d_wpred, d_partial);
    else return hipErrorInvalidValue;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (cols == 3) hipLaunchKernelGGL(pose_finish, dim3((NB * 6 + 63) / 64), dim3(64), 0, s, d_partial, NB, P, d_bpred, d_pose, sel);
    else if (heads == 2) hipLaunchKernelGGL(pose_finish6, dim3((NB * 12 + 63) / 64), dim3(64), 0, s, d_partial, NB, P, d_bpred, d_pose);
    else hipLaunchKernelGGL(pose_finish_coupled, dim3((NB * 6 + 63) / 64), dim3(64), 0, s, d_partial, NB, P, d_bpred, d_pose, sel);
    return hipGetLastError();
}

hipError_t launch_conv_direct(const float* x, int N, int Hin, int Win, int cin, int x_ld, int x_coff, const float* w, int KS,
                              int cout, const float* bias, int stride, int rate, int pt, int pl, int Ho, int Wo, int relu,
                              float* y, int y_ld, int y_coff, hipStream_t s) {
    const long total = (long)N * Ho * Wo * cout;
    hipLaunchKernelGGL(conv_direct, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, N, Hin, Win, cin, x_ld, x_coff,
                       w, KS, cout, bias, stride, rate, pt, pl, Ho, Wo, relu, y, y_ld, y_coff);
    return hipGetLastError();
}

hipError_t launch_se5_squeeze(bool h3, const void* d_x, int NB, int P, float* d_partial, hipStream_t s) {
    if (NB < 1 || P < 1 || !d_x || !d_partial) return hipErrorInvalidValue;
    const uint8_t* x = static_cast<const uint8_t*>(d_x);
    if (h3) hipLaunchKernelGGL(se5_squeeze<true>, dim3(SE5_CHUNKS, NB), dim3(256), 0, s, x, P, d_partial);
    else hipLaunchKernelGGL(se5_squeeze<false>, dim3(SE5_CHUNKS, NB), dim3(256), 0, s, x, P, d_partial);
    return hipGetLastError();
}

hipError_t launch_se5_excite(const float* d_partial, int NB, int P, float unscale, const SeDense& rot, const SeDense& trans, float* d_scale, hipStream_t s) {
    if (NB < 1 || P < 1 || !d_partial || !d_scale || !rot || !trans) return hipErrorInvalidValue;
    const Se5Weights w{rot.w1, rot.b1, rot.w2, rot.b2, trans.w1, trans.b1, trans.w2, trans.b2};
    hipLaunchKernelGGL(se5_excite, dim3(NB), dim3(256), 0, s, d_partial, P, unscale, w, d_scale);
    return hipGetLastError();
}

hipError_t launch_se5_scale(bool h3, const void* d_x, const float* d_scale, int NB, int P, void* d_y, unsigned* d_range, hipStream_t s) {
    if (NB < 1 || P < 1 || !d_x || !d_scale || !d_y) return hipErrorInvalidValue;
    const uint8_t* x = static_cast<const uint8_t*>(d_x);
    uint8_t* y = static_cast<uint8_t*>(d_y);
    const dim3 grid((unsigned)(((long)P * (h3 ? 32 : 64) + 255) / 256), NB);
    if (h3) hipLaunchKernelGGL(se5_scale<true>, grid, dim3(256), 0, s, x, d_scale, P, y, d_range);
    else hipLaunchKernelGGL(se5_scale<false>, grid, dim3(256), 0, s, x, d_scale, P, y, d_range);
    return hipGetLastError();
}

}  // namespace davo
