// gemm_ops.hip -- launchers that map conv / linear layers (fwd, dgrad, wgrad) onto igemm tiles,
// plus the small HBM-bound helpers around them (weight repack, column sums for bias gradients).
#include "igemm.h"
#include "igemm_dma.h"
#include "igemm_dma_wgrad.h"
#include "igemm_bf3.h"
#include "igemm_bf3_ws.h"
#include "dense_bf3.h"
#include "obs_conv_bf3.h"
#include "obs_conv_bf3_ws.h"
#include "obs_conv_patch.h"
#include "wgrad3x3_bf3.h"
#include "conv2_fwd_strip.h"
#include "conv2_dgrad_strip.h"
#include "conv3_dgrad_strip.h"
#include "obs_wgrad_bf3.h"
#include "obs_wgrad_strip.h"
#include "conv_patch_bf3.h"
#include "wgrad3x3_patch.h"
#include "prob_build.h"
#include <stdlib.h>

#include <atomic>

#include "../../include/habitat_amd.h"

namespace hab {

// The mask of hab_set_matrix_path (env HAB_BF3): which contractions run on the split-bf16 matrix-pipe kernels and in which form.
// ops.h names the bits (MatrixPath), include/habitat_amd.h describes them.
static std::atomic<int> g_bf3_mode{-1};  // engines of several inference-worker threads dispatch concurrently
int matrix_path_bits() {
    int m = g_bf3_mode.load(std::memory_order_relaxed);
    if (m < 0) {
        static const int from_env = hab_env_int("HAB_BF3", MP_DEFAULT);
        int expected = -1;
        g_bf3_mode.compare_exchange_strong(expected, from_env, std::memory_order_relaxed);
        m = g_bf3_mode.load(std::memory_order_relaxed);
    }
    return m;
}
extern "C" int hab_set_matrix_path(int mode) {
    const int prev = matrix_path_bits();
    if (mode >= 0) g_bf3_mode.store(mode, std::memory_order_relaxed);
    return prev;
}

// Tile choice by output width N (= Cout / out-features) and height M: tall-skinny tiles because the policy's
// layers have N in 32..512 and M in 1e2..1e7.  Weight-gradient problems have small M x N and a
// huge reduction: the 96-row tile (3 waves) avoids padding M = 288 / 576 / 1152 (3x3 taps x 32..128 channels).
template <int TM_, int TN_, int WM_, int WN_>
struct Tile {  // TM x TN MFMA blocks of 32 x 32 per wave, WM x WN waves
    static constexpr int TM = TM_, TN = TN_, WM = WM_, WN = WN_;
};
using Tile128x128 = Tile<2, 2, 2, 2>;
// tiles of `rows` rows pad M less than tiles of `other` rows do (or not at all)
static bool rows_fit(int M, int rows, int other) { return M % rows == 0 || cdiv(M, rows) * rows < cdiv(M, other) * other; }
// The width classes of every tile family (split-bf16, LDS-DMA, fp32, merged data gradient): launch(Tile<...>{}) for the class of N;
// WG (weight-gradient problems) adds the 96-row tiles.  A family instantiates its kernel for the tiles named here under its WG and
// for those it names itself, no others.
template <bool WG, class F>
static int by_width(int M, int N, F launch) {
    if (N <= 32) {
        if constexpr (WG) {
            if (rows_fit(M, 96, 256)) return launch(Tile<1, 1, 3, 1>{});
        }
        return launch(Tile<2, 1, 4, 1>{});
    }
    if (N <= 64) {
        if constexpr (WG) {
            if (rows_fit(M, 96, 128)) return launch(Tile<1, 2, 3, 1>{});
        }
        return launch(Tile<1, 2, 4, 1>{});
    }
    return launch(Tile128x128{});
}

// Producer / consumer waves (igemm_bf3_ws.h, MP_WS, on by default).  Measured on the MI355X against igemm_bf3_kernel, same
// arithmetic and bit-identical results (profiles/r03_ws_vs_base_layers.txt): the 128 x 128 forward-form tiles with a long reduction gain
// (3x3 256->256 at 4x4: 128 -> 163 TFLOP/s-eq forward and data gradient, fc 25088->512 forward 132 -> 150), every other shape loses
// (32- / 64-column tiles -10..-45 %, i/j-contiguous operands -30 %, K = 256 merged data gradient -18 %: the longer prologue and the
// halved MFMA wave count are not paid back).  It is therefore selected only where it won.
template <class P, class T>
static int bf3_launch(const P& p, float* ws, size_t ws_floats, int target_blocks, hipStream_t stream) {
    if constexpr (P::A_RC && P::B_RC && std::is_same_v<T, Tile128x128>) {
        constexpr int ws_min_k = 2048;
        if (matrix_path_on(MP_WS) && p.K >= ws_min_k) return igemm_bf3_ws_launch<P, T::TM, T::TN, T::WM, T::WN, 4>(p, ws, ws_floats, target_blocks, stream);
    }
    return igemm_bf3_launch<P, T::TM, T::TN, T::WM, T::WN>(p, ws, ws_floats, target_blocks, stream);
}
// LDS-DMA staged variant (igemm_dma.h).  DB_WIDE: the 128 x 128 tile double-buffers its LDS stage.
template <bool DB_WIDE, class P>
static int dma_launch(const P& p, float* ws, size_t ws_floats, int target_blocks, hipStream_t stream) {
    return by_width<false>(p.M, p.N, [&](auto t) {
        using T = decltype(t);
        return igemm_dma_launch<P, T::TM, T::TN, T::WM, T::WN, DB_WIDE && std::is_same_v<T, Tile128x128>>(p, ws, ws_floats, target_blocks, stream);
    });
}

template <class P>
static int run_igemm(const P& p, float* ws, size_t ws_floats, hipStream_t stream, int target_blocks = 1024) {
    // Split-K target.  Forward-form problems (activations x weights) split only until there is one workgroup per CU: their
    // split-K second pass re-reads M*N*splits floats and, at rollout batch sizes, costs more than the idle CUs it fills
    // (measured: target 1024 -> 256 is +4 % on C2, +6 % on C3, all of it in the 64-frame rollout forward passes).  Weight
    // gradients (tiny M*N, K in the millions) keep the deeper split.
    if (P::A_RC || P::B_RC) target_blocks = 256;
    constexpr bool RC = P::A_RC && P::B_RC;                                 // both operands r-contiguous
    constexpr bool IJ = !RC && AKv<P>::value == 4;                          // an i/j-contiguous operand: register-transposed staging (igemm_bf3.h)
    constexpr bool WG = !P::A_RC && !P::B_RC && AKv<P>::value == 4;  // weight-gradient form
    if constexpr (RC || IJ) {
        if (matrix_path_on(RC ? MP_RC : MP_IJ) && p.M > 64) {
            if constexpr (RC) {
                // 256 x 64 tiles halve the weight traffic per output row: +12 % on the 3x3 64 -> 64 convolutions of ResNet layer2
                // (0.089 -> 0.079 ms at 512 frames, forward and data gradient), nothing on SimpleCNN conv2 (K = 512: 0.308 vs 0.312 ms)
                if (p.N > 32 && p.N <= 64 && p.M >= 256 * 512 && p.K >= 576) return bf3_launch<P, Tile<2, 2, 4, 1>>(p, ws, ws_floats, target_blocks, stream);
            }
            return by_width<WG>(p.M, p.N, [&](auto t) { return bf3_launch<P, decltype(t)>(p, ws, ws_floats, target_blocks, stream); });
        }
    }
    if constexpr (std::is_same_v<P, ConvFwdProb> || std::is_same_v<P, ConvDgradProb>) {
        if (p.dma_ok() && p.M > 64 && p.N <= 128) return dma_launch<true>(p, ws, ws_floats, target_blocks, stream);
    }
    if (p.M <= 64) {
        if (p.N <= 32) return igemm_launch<P, 1, 1, 2, 1>(p, ws, ws_floats, target_blocks, stream);
        if (p.N <= 64) return igemm_launch<P, 1, 1, 2, 2>(p, ws, ws_floats, target_blocks, stream);
        return igemm_launch<P, 1, 2, 2, 2>(p, ws, ws_floats, target_blocks, stream);
    }
    return by_width<WG>(p.M, p.N, [&](auto t) {
        using T = decltype(t);
        return igemm_launch<P, T::TM, T::TN, T::WM, T::WN>(p, ws, ws_floats, target_blocks, stream);
    });
}

// Stride-1 3x3 convolutions with the input patch resident in LDS (conv_patch_bf3.h, MP_PATCH3X3): `in` is x for the forward and dY,
// with the taps flipped, for the data gradient; off is the input offset of tap 0 relative to the output pixel.
static bool patch3x3_wanted(const ConvDesc& d, int M) { return matrix_path_on(MP_PATCH3X3) && d.stride == 1 && d.KH == 3 && d.KW == 3 && M > 64; }
static PatchGeom patch3x3_geom(const float* in, int Hi, int Wi, int Ci, int Ho, int Wo, int off, int flip) {
    PatchGeom gq{};
    gq.in = in; gq.Hi = Hi; gq.Wi = Wi; gq.Ci = Ci; gq.Ho = Ho; gq.Wo = Wo; gq.KH = 3; gq.KW = 3;
    gq.off_h = off; gq.off_w = off; gq.flip = flip;
    return gq;
}

// The form of a convolution's forward (HAB_CONV_FWD_FORM_*): under MP_CONV2_FWD with MP_RC SimpleCNN's conv2 on its strip kernel (input
// strip in LDS, filter slices in registers: conv2_fwd_strip.h) where that serves the call -- folded, or under MP_CONV2_STRIP_PLAIN plain;
// the two give equal bits -- and the general kernels for everything else.  conv_fwd and hab_conv2d_fwd_form both ask it.
static int choose_conv_fwd(const ConvFwdProb& p) {
    if (!matrix_path_on(MP_CONV2_FWD | MP_RC) || !conv2_fwd_strip_serves(p)) return HAB_CONV_FWD_FORM_GENERAL;
    return matrix_path_on(MP_CONV2_STRIP_PLAIN) ? HAB_CONV_FWD_FORM_CONV2_STRIP_PLAIN : HAB_CONV_FWD_FORM_CONV2_STRIP;
}
int conv_fwd(const ConvDesc& d, const float* x, const float* wf, const float* bias, float* y, int relu, float* ws,
             size_t ws_floats, hipStream_t stream) {
    ConvFwdProb p;
    HAB_TRY(build(p, d, x, wf, bias, y, relu));
    const int form = choose_conv_fwd(p);
    if (form != HAB_CONV_FWD_FORM_GENERAL) HAB_TRY_FORM(conv2_fwd_strip(p, form == HAB_CONV_FWD_FORM_CONV2_STRIP, stream));
    if (patch3x3_wanted(d, p.M))
        HAB_TRY_FORM(conv_patch_bf3_dispatch(p, patch3x3_geom(x, d.H, d.W, d.C, p.g.Ho, p.g.Wo, -d.pad, 0), ws, ws_floats, stream));
    return run_igemm(p, ws, ws_floats, stream);
}
int64_t obs_conv_weight_image_floats() { return ((int64_t)OCP_W_ELEMS + 1) / 2 + 4; }
int obs_conv_weight_image(const float* wf, int Cout, int KH, int KW, int C, void* img, hipStream_t stream) {
    return obs_conv_patch_weight_image(wf, Cout, KH, KW, C, reinterpret_cast<unsigned short*>(img), stream);
}
// Whether conv1's forward runs with the observation patch resident in LDS (obs_conv_patch.h, MP_OBS_PATCH with MP_OBS: 8x8 / 4 RGB-D -> at
// most 32 channels), and in which form of that kernel (HAB_OBS_FWD_FORM_*): the hoisted one, or under MP_OBS_PATCH_PLAIN the plain one.
// OTHER: the im2col kernels / igemm tiles below.  obs_conv_fwd and hab_obs_conv2d_fwd_form both ask it.
static int choose_obs_fwd(const ObsConvFwdProb& p, const float* ws, size_t ws_floats, const void* wimg) {
    if (!(matrix_path_on(MP_OBS_PATCH | MP_OBS) && obs_conv_patch_covers(p, ws, ws_floats, reinterpret_cast<const unsigned short*>(wimg))))
        return HAB_OBS_FWD_FORM_OTHER;
    return matrix_path_on(MP_OBS_PATCH_PLAIN) ? HAB_OBS_FWD_FORM_PATCH_PLAIN : HAB_OBS_FWD_FORM_PATCH;
}
int obs_conv_fwd(const ConvDesc& d, const ObsView& obs, const float* wf, const float* bias, float* y, int relu, float* ws,
                 size_t ws_floats, hipStream_t stream, const void* wimg) {
    ObsConvFwdProb p;
    HAB_TRY(build(p, d, obs, wf, bias, y, relu));
    const int form = choose_obs_fwd(p, ws, ws_floats, wimg);
    if (form != HAB_OBS_FWD_FORM_OTHER)
        HAB_TRY_FORM(obs_conv_patch_launch(p, ws, ws_floats, stream, reinterpret_cast<const unsigned short*>(wimg), form == HAB_OBS_FWD_FORM_PATCH));
    if (matrix_path_on(MP_WS | MP_OBS) && p.quad && p.M > 64)  // producer / consumer waves (obs_conv_bf3_ws.h): 133 -> 148-152 TFLOP/s-eq at 1024 frames
        HAB_TRY_FORM(obs_conv_bf3_ws_launch(p, ws, ws_floats, stream));
    if (matrix_path_on(MP_OBS) && p.quad && p.M > 64)  // uint8 x split-bf16 weights on the matrix pipe (obs_conv_bf3.h)
        HAB_TRY_FORM(obs_conv_bf3_launch<2>(p, ws, ws_floats, stream));
    return run_igemm(p, ws, ws_floats, stream);
}
// dX pixels whose class has no taps (possible only when stride > kernel size) receive no contribution:
// they are written by the zero-tap path below so that dx is always fully defined.
__global__ void dgrad_empty_class_kernel(ConvDgradProb p) {
    const long long total = (long long)p.g.B * p.Hc * p.Wc * p.N;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
        p.store((int)(e / p.N), (int)(e % p.N), 0.f);
}

// The form of a convolution's data gradient (HAB_CONV_DGRAD_FORM_*): under MP_CONV2_DGRAD with MP_RC SimpleCNN's conv2 and conv3 on their
// strip kernels (dY strip in LDS, filter slices in registers: conv2_dgrad_strip.h, conv3_dgrad_strip.h) where those serve the call, the
// general kernels (patch-resident 3x3, merged stride classes, igemm tiles) for everything else.  conv_dgrad and hab_conv2d_dgrad_form
// both ask it.
static int choose_conv_dgrad(const ConvDesc& d, const float* dy, const float* wd, const float* mask, const float* add, const float* dx) {
    if (!matrix_path_on(MP_CONV2_DGRAD | MP_RC)) return HAB_CONV_DGRAD_FORM_GENERAL;
    if (conv2_dgrad_strip_serves(d, dy, wd, mask, add, dx))  // folded, or under MP_CONV2_STRIP_PLAIN plain: equal bits
        return matrix_path_on(MP_CONV2_STRIP_PLAIN) ? HAB_CONV_DGRAD_FORM_CONV2_STRIP_PLAIN : HAB_CONV_DGRAD_FORM_CONV2_STRIP;
    if (conv3_dgrad_strip_serves(d, dy, wd, mask, add, dx)) return HAB_CONV_DGRAD_FORM_CONV3_STRIP;
    return HAB_CONV_DGRAD_FORM_GENERAL;
}
int conv_dgrad(const ConvDesc& d, const float* dy, const float* wd, const float* mask, const float* add, float* dx,
               float* ws, size_t ws_floats, hipStream_t stream) {
    const int form = choose_conv_dgrad(d, dy, wd, mask, add, dx);
    if (form == HAB_CONV_DGRAD_FORM_CONV2_STRIP || form == HAB_CONV_DGRAD_FORM_CONV2_STRIP_PLAIN)
        HAB_TRY_FORM(conv2_dgrad_strip(d, dy, wd, mask, add, dx, form == HAB_CONV_DGRAD_FORM_CONV2_STRIP, stream));
    if (form == HAB_CONV_DGRAD_FORM_CONV3_STRIP) HAB_TRY_FORM(conv3_dgrad_strip(d, dy, wd, mask, add, dx, stream));
    if (d.stride > 1) {
        // kernel size a multiple of the stride: the stride classes share their dY gather -> one contraction with N = s*s*Cin
        ConvDgradMergedProb q;
        HAB_TRY(check_conv(d));
        q.g = make_geom(d);
        if (ConvDgradMergedProb::applicable(q.g)) {
            q.dy = dy; q.w = wd; q.mask = mask; q.add = add; q.dx = dx;
            q.finish();
            if (matrix_path_on(MP_RC) && q.M > 64)  // split-bf16 matrix path, register-staged (igemm_bf3.h)
                return by_width<false>(q.M, q.N, [&](auto t) { return bf3_launch<ConvDgradMergedProb, decltype(t)>(q, ws, ws_floats, 256, stream); });
            // single LDS buffer at every width: K is short (KH/s * KW/s taps), 4 resident workgroups overlap each other's prologue / epilogue
            // (measured 79 vs 68 TFLOP/s double-buffered on SimpleCNN conv2 with the ReLU-mask epilogue)
            if (q.dma_ok()) return dma_launch<false>(q, ws, ws_floats, 1024, stream);
        }
    }
    for (int ph = 0; ph < d.stride; ++ph)
        for (int pw = 0; pw < d.stride; ++pw) {
            ConvDgradProb p;
            HAB_TRY(build(p, d, dy, wd, mask, add, dx, ph, pw));
            if (p.Hc <= 0 || p.Wc <= 0) continue;
            if (patch3x3_wanted(d, p.M) && p.K > 0) {
                const int rc = conv_patch_bf3_dispatch(p, patch3x3_geom(dy, p.g.Ho, p.g.Wo, d.Cout, d.H, d.W, d.pad - 2, 1), ws, ws_floats, stream);
                if (rc == HAB_OK) continue;
                if (rc != HAB_NOT_APPLICABLE) return rc;
            }
            if (p.K <= 0) {
                p.M = d.B * p.Hc * p.Wc;
                dgrad_empty_class_kernel<<<1024, 256, 0, stream>>>(p);
                HAB_LAUNCH_CHECK();
                continue;
            }
            HAB_TRY(run_igemm(p, ws, ws_floats, stream));
        }
    return HAB_OK;
}
int conv_wgrad(const ConvDesc& d, const float* x, const float* dy, float* dw_oihw, float* dbias, float* ws, size_t ws_floats,
               hipStream_t stream) {
    ConvWgradProb p;
    HAB_TRY(build(p, d, x, dy, dw_oihw, dbias));
    if (ws && matrix_path_on(MP_WGRAD_STRIP | MP_IJ_WGRAD) && wgrad3x3_bf3_shape(p))  // strip-resident, transpose reads (wgrad3x3_bf3.h)
        HAB_TRY_FORM(wgrad3x3_bf3(p, ws, ws_floats, stream));
    if (ws && !matrix_path_on(MP_IJ_WGRAD)) {
        // the fp32 patch / LDS-DMA kernels never see dY in registers: they take the problem without `colsum`, the bias gradient is a
        // separate column sum
        ConvWgradProb q = p;
        q.colsum = nullptr;
        auto bias_grad = [&] { return dbias ? colsum(dy, p.N, p.K, p.N, dbias, 0, ws, ws_floats, stream) : HAB_OK; };
        // A workspace too short for a form declines the form, it does not fail the call (the igemm tiles below need none and fuse the bias
        // gradient).  Decided before anything is launched: the column sum needs one row of N floats, the patch kernel one slab.
        const bool bias_fits = !dbias || ws_floats >= (size_t)p.N;
        if (bias_fits && wgrad3x3_patch_ok(p) && wgrad3x3_patch_fits(p, ws_floats)) {  // 3x3/1/1 with W in {16, 32}: patch-resident kernel
            HAB_TRY(bias_grad());
            return wgrad3x3_patch(q, ws, ws_floats, stream);
        }
        // LDS-DMA staged variant (igemm_dma_wgrad.h): measured faster only for unpadded convolutions with Cout <= 32 (SimpleCNN conv3:
        // 51 -> 64 TFLOP/s); with padding the per-pixel scalar decode + border tests cost more than the VGPR staging they replace.
        if (bias_fits && d.pad == 0 && p.N <= 32 && wgrad_dma_ok(q)) {
            HAB_TRY(bias_grad());
            if (rows_fit(q.M, 288, 256)) return igemm_dma_wgrad_launch<3, 3, 1>(q, ws, ws_floats, 1024, stream);
            return igemm_dma_wgrad_launch<2, 4, 1>(q, ws, ws_floats, 1024, stream);
        }
    }
    return run_igemm(p, ws, ws_floats, stream);
}
// The form of conv1's weight gradient for a problem and workspace (HAB_OBS_WGRAD_FORM_*): uint8 x split-bf16 dY on the matrix pipe
// under MP_OBS for more than 4096 output pixels -- with MP_OBS_PATCH the observation rows resident in LDS (obs_wgrad_strip.h), else or
// where that form does not cover the geometry the im2col gather (obs_wgrad_bf3.h) -- and the igemm tiles for everything else.
// obs_conv_wgrad and hab_obs_conv2d_wgrad_form both ask it.
static int choose_obs_wgrad(const ObsConvWgradProb& p, const float* ws, size_t ws_floats) {
    if (!(matrix_path_on(MP_OBS) && p.quad && p.K > 4096)) return HAB_OBS_WGRAD_FORM_IGEMM;
    if (matrix_path_on(MP_OBS_PATCH | MP_OBS) && obs_wgrad_strip_covers(p, ws, ws_floats)) return HAB_OBS_WGRAD_FORM_STRIP;
    return obs_wgrad_bf3_covers(p, ws, ws_floats) ? HAB_OBS_WGRAD_FORM_IM2COL : HAB_OBS_WGRAD_FORM_IGEMM;
}
int obs_conv_wgrad(const ConvDesc& d, const ObsView& obs, const float* dy, float* dw_oihw, float* dbias, float* ws,
                   size_t ws_floats, hipStream_t stream) {
    ObsConvWgradProb p;
    HAB_TRY(build(p, d, obs, dy, dw_oihw, dbias));
    const int form = choose_obs_wgrad(p, ws, ws_floats);
    if (form == HAB_OBS_WGRAD_FORM_STRIP) HAB_TRY_FORM(obs_wgrad_strip_launch(p, ws, ws_floats, stream));
    if (form >= HAB_OBS_WGRAD_FORM_IM2COL) HAB_TRY_FORM(obs_wgrad_bf3_launch(p, ws, ws_floats, stream));
    return run_igemm(p, ws, ws_floats, stream);
}

// Large Linear layers on the plain dense GEMM kernel (dense_bf3.h, MP_DENSE with MP_RC).
static bool dense_wanted(long long M, long long N, long long K) {
    if (!matrix_path_on(MP_DENSE | MP_RC)) return false;
    if (matrix_path_on(MP_DENSE_ALL)) return true;  // (tests) every applicable shape
    // the shapes it was built and measured for: >= ~10 GFLOP contractions (SimpleCNN's visual fc and its gradients); smaller layers keep
    // the igemm tiles (their launch is shorter than this kernel's 256 x 128 x K prologue / epilogue)
    static const long long min_flop = (long long)hab_env_int("HAB_DENSE_MIN_MFLOP", 4000) * 1000000LL;
    return 2 * M * N * K >= min_flop;
}
// g: the operands and epilogue of C[M][N] = A B^T; p: the same layer as an igemm problem, whose reduction pass sums the split-K slabs.
// HAB_NOT_APPLICABLE: the caller runs the igemm tiles.
template <int A_IC, int B_IC, class P>
static int dense_try(DenseArgs g, const P& p, float* ws, size_t ws_floats, hipStream_t stream) {
    if (!dense_wanted(g.M, g.N, g.K) || !dense_bf3_ok(g, A_IC, B_IC)) return HAB_NOT_APPLICABLE;
    g.partial = ws;
    g.nsplit = ws ? dense_bf3_splits(g, ws_floats) : 1;
    HAB_TRY((dense_bf3_launch<A_IC, B_IC>(g, stream)));
    if (g.nsplit > 1) {
        igemm_splitk_reduce<P>(p, ws, g.nsplit, stream);
        HAB_LAUNCH_CHECK();
    }
    return HAB_OK;
}
int linear_fwd(const float* x, int ldx, const float* w, int ldw, const float* bias, float* y, int ldy, int M, int N, int K,
               int relu, int accumulate, float* ws, size_t ws_floats, hipStream_t stream) {
    LinearFwdProb p;
    HAB_TRY(build(p, x, ldx, w, ldw, bias, y, ldy, M, N, K, relu, accumulate));
    DenseArgs g{};
    g.M = M; g.N = N; g.K = K; g.a = x; g.lda = ldx; g.b = w; g.ldb = ldw; g.c = y; g.ldc = ldy; g.bias = bias; g.relu = relu;
    g.accumulate = accumulate;
    g.a_bytes = ((long long)(M - 1) * ldx + K) * 4; g.b_bytes = ((long long)(N - 1) * ldw + K) * 4;
    HAB_TRY_FORM((dense_try<0, 0>(g, p, ws, ws_floats, stream)));
    return run_igemm(p, ws, ws_floats, stream);
}
int linear_dgrad(const float* dy, int lddy, const float* w, int ldw, const float* mask, int ldmask, int mask_cols, float* dx,
                 int lddx, int M, int Nin, int Kout, int accumulate, float* ws, size_t ws_floats, hipStream_t stream) {
    LinearDgradProb p;
    HAB_TRY(build(p, dy, lddy, w, ldw, mask, ldmask, mask_cols, dx, lddx, M, Nin, Kout, accumulate));
    if (!mask) {  // dX[M][Nin] = dY[M][Kout] W[Kout][Nin]: W is the k-strided operand
        DenseArgs g{};
        g.M = M; g.N = Nin; g.K = Kout; g.a = dy; g.lda = lddy; g.b = w; g.ldb = ldw; g.c = dx; g.ldc = lddx; g.accumulate = accumulate;
        g.a_bytes = ((long long)(M - 1) * lddy + Kout) * 4; g.b_bytes = ((long long)(Kout - 1) * ldw + Nin) * 4;
        HAB_TRY_FORM((dense_try<0, 1>(g, p, ws, ws_floats, stream)));
    }
    return run_igemm(p, ws, ws_floats, stream);
}
int linear_wgrad(const float* dy, int lddy, const float* x, int ldx, float* dw, int lddw, int Mrows, int Nout, int Kin,
                 int perm_c, int perm_hw, int accumulate, float* ws, size_t ws_floats, hipStream_t stream) {
    LinearWgradProb p;
    HAB_TRY(build(p, dy, lddy, x, ldx, dw, lddw, Mrows, Nout, Kin, perm_c, perm_hw, accumulate));
    // dW[Nout][Kin] = dY^T X: both operands are indexed by the frame = k-strided (the reduction pass applies the flatten permutation and
    // `accumulate`: LinearWgradProb::store)
    DenseArgs g{};
    g.M = Nout; g.N = Kin; g.K = Mrows; g.a = dy; g.lda = lddy; g.b = x; g.ldb = ldx; g.c = dw; g.ldc = lddw; g.accumulate = accumulate;
    g.perm_c = perm_c; g.perm_hw = perm_hw;
    g.a_bytes = ((long long)(Mrows - 1) * lddy + Nout) * 4; g.b_bytes = ((long long)(Mrows - 1) * ldx + Kin) * 4;
    HAB_TRY_FORM((dense_try<1, 1>(g, p, ws, ws_floats, stream)));
    return run_igemm(p, ws, ws_floats, stream);
}

// ---------------------------------------------------------------------------------------------
// Column sums (bias gradients): out[n] = sum_m a[m][n] * (mask ? mask[m][n] > 0 : 1).
// Stage 1: each block reduces a row range into partial[block][N]; stage 2: fixed-order sum.
// ---------------------------------------------------------------------------------------------
// grid = (column blocks of cw = min(64, N) columns, row chunks); 256 threads = (256 / cw) row lanes x cw columns.
__global__ void __launch_bounds__(256) colsum_stage1(const float* __restrict__ a, int lda, int M, int N, int rows_per_block,
                                                     float* __restrict__ partial) {
    const int cw = N < 64 ? N : 64;
    const int rl = 256 / cw;
    const int c = threadIdx.x % cw, r = threadIdx.x / cw;
    const int n = blockIdx.x * cw + c;
    __shared__ float sm[256];
    const int m_begin = blockIdx.y * rows_per_block, m_end = min(M, m_begin + rows_per_block);
    float s0 = 0.f, s1 = 0.f;
    if (r < rl && n < N) {
        int m = m_begin + r;
        for (; m + rl < m_end; m += 2 * rl) {
            s0 += a[(size_t)m * lda + n];
            s1 += a[(size_t)(m + rl) * lda + n];
        }
        if (m < m_end) s0 += a[(size_t)m * lda + n];
    }
    sm[threadIdx.x] = s0 + s1;
    __syncthreads();
    if (r == 0 && n < N) {
        float t = 0.f;
        for (int q = 0; q < rl; ++q) t += sm[q * cw + c];
        partial[(size_t)blockIdx.y * N + n] = t;
    }
}
__global__ void __launch_bounds__(256) colsum_stage2(const float* __restrict__ partial, int nblocks, int N, float* __restrict__ out,
                                                     int accumulate) {
    // 64 columns per block, 4 row lanes
    __shared__ float sm[4][64];
    const int c = threadIdx.x & 63, r = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    // four independent chains per row lane: up to 64 partials per lane were one dependent chain of L2 round trips (15 us for a 32-column
    // sum that moves 32 KB; 80 such launches per ResNet18 minibatch, 200 per ResNet50 one)
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (n < N) {
        int b = r;
        for (; b + 12 < nblocks; b += 16) {
            s0 += partial[(size_t)b * N + n];
            s1 += partial[(size_t)(b + 4) * N + n];
            s2 += partial[(size_t)(b + 8) * N + n];
            s3 += partial[(size_t)(b + 12) * N + n];
        }
        for (; b < nblocks; b += 4) s0 += partial[(size_t)b * N + n];
    }
    const float s = (s0 + s1) + (s2 + s3);
    sm[r][c] = s;
    __syncthreads();
    if (r == 0 && n < N) {
        const float t = (sm[0][c] + sm[1][c]) + (sm[2][c] + sm[3][c]);
        out[n] = accumulate ? out[n] + t : t;
    }
}

int colsum(const float* a, int lda, int M, int N, float* out, int accumulate, float* ws, size_t ws_floats, hipStream_t stream) {
    if (M <= 0 || N <= 0 || !a || !out || !ws) return HAB_ERR_ARG;
    const int cw = N < 64 ? N : 64;
    const int colblocks = cdiv(N, cw);
    // enough row chunks for ~1024 workgroups, at least 16 rows each
    int chunks = cdiv(1024, colblocks);
    if (chunks > cdiv(M, 16)) chunks = cdiv(M, 16);
    while (chunks > 1 && (size_t)chunks * N > ws_floats) chunks >>= 1;
    if ((size_t)chunks * N > ws_floats) return HAB_ERR_ARG;
    const int rpb = cdiv(M, chunks);
    chunks = cdiv(M, rpb);
    colsum_stage1<<<dim3(colblocks, chunks), 256, 0, stream>>>(a, lda, M, N, rpb, ws);
    HAB_LAUNCH_CHECK();
    colsum_stage2<<<cdiv(N, 64), 256, 0, stream>>>(ws, chunks, N, out, accumulate);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

// ---------------------------------------------------------------------------------------------
// Weight repack: OIHW master -> Wf[co][(kh,kw,ci)] and Wd[ci][(kh,kw,co)].  cpad >= Cin pads the
// packed input-channel dimension with zeros (stem conv: 4/5 obs channels -> 4/8).
// ---------------------------------------------------------------------------------------------
__global__ void repack_conv_kernel(const float* __restrict__ w, float* __restrict__ wf, float* __restrict__ wd, int Cout,
                                   int Cin, int KH, int KW, int cpad) {
    const int total = Cout * cpad * KH * KW;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        // e enumerates Wf: [co][kh][kw][ci(cpad)]
        const int ci = e % cpad;
        int t = e / cpad;
        const int kw = t % KW; t /= KW;
        const int kh = t % KH;
        const int co = t / KH;
        const float v = (ci < Cin) ? w[(((size_t)co * Cin + ci) * KH + kh) * KW + kw] : 0.f;
        if (wf) wf[e] = v;
        if (wd && ci < Cin) wd[(((size_t)ci * KH + kh) * KW + kw) * Cout + co] = v;
    }
}

int repack_conv(const float* w_oihw, float* wf, float* wd, int Cout, int Cin, int KH, int KW, int cpad, hipStream_t stream) {
    if (!w_oihw || Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0 || cpad < Cin) return HAB_ERR_ARG;
    if (wd && cpad != Cin) return HAB_ERR_UNSUPPORTED;
    const int total = Cout * cpad * KH * KW;
    repack_conv_kernel<<<min(1024, cdiv(total, 256)), 256, 0, stream>>>(w_oihw, wf, wd, Cout, Cin, KH, KW, cpad);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

// Linear weight after nn.Flatten of an NCHW tensor: Wp[n][hw*C + c] = W[n][c*HW + hw].
__global__ void repack_flatten_kernel(const float* __restrict__ w, float* __restrict__ wp, int N, int C, int HW) {
    const size_t total = (size_t)N * C * HW;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const size_t t = e / C;
        const int hw = (int)(t % HW);
        const size_t n = t / HW;
        wp[e] = w[(n * C + c) * HW + hw];
    }
}
int repack_flatten(const float* w, float* wp, int N, int C, int HW, hipStream_t stream) {
    if (!w || !wp || N <= 0 || C <= 0 || HW <= 0) return HAB_ERR_ARG;
    const size_t total = (size_t)N * C * HW;
    repack_flatten_kernel<<<(int)fmin(4096.0, (double)cdivl((long long)total, 256)), 256, 0, stream>>>(w, wp, N, C, HW);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

// Transposed copy: wt[c][r] = w[r][c]   (RNN recurrent weights for the BPTT mat-vec)
__global__ void transpose_kernel(const float* __restrict__ w, float* __restrict__ wt, int R, int C) {
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int r = by + j, c = bx + threadIdx.x;
        tile[j][threadIdx.x] = (r < R && c < C) ? w[(size_t)r * C + c] : 0.f;
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int c = bx + j, r = by + threadIdx.x;
        if (c < C && r < R) wt[(size_t)c * R + r] = tile[threadIdx.x][j];
    }
}
__global__ void pad_rows_kernel(const float* __restrict__ w, float* __restrict__ wp, int R, int C, int ld) {
    const long long total = (long long)R * ld;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(e % ld);
        const long long r = e / ld;
        wp[e] = c < C ? w[r * C + c] : 0.f;
    }
}
int pad_rows(const float* w, float* wp, int R, int C, int ld, hipStream_t stream) {
    if (!w || !wp || R <= 0 || C <= 0 || ld < C) return HAB_ERR_ARG;
    const long long total = (long long)R * ld;
    pad_rows_kernel<<<(int)fmin(2048.0, (double)cdivl(total, 256)), 256, 0, stream>>>(w, wp, R, C, ld);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}
int transpose2d(const float* w, float* wt, int R, int C, hipStream_t stream) {
    if (!w || !wt || R <= 0 || C <= 0) return HAB_ERR_ARG;
    transpose_kernel<<<dim3(cdiv(C, 32), cdiv(R, 32)), dim3(32, 8), 0, stream>>>(w, wt, R, C);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

}  // namespace hab

// ------------------------------------------- C ABI -------------------------------------------
using namespace hab;

static ConvDesc mk(int B, int H, int W, int C, int Cout, int KH, int KW, int stride, int pad) {
    ConvDesc d;
    d.B = B; d.H = H; d.W = W; d.C = C; d.Cout = Cout; d.KH = KH; d.KW = KW; d.stride = stride; d.pad = pad;
    return d;
}
static ObsView mkobs(const uint8_t* rgb, const float* depth, const int* rows, int H, int W) {
    ObsView o;
    o.rgb = rgb; o.depth = depth; o.rows = rows; o.H = H; o.W = W; o.C = (rgb ? 3 : 0) + (depth ? 1 : 0);
    return o;
}

extern "C" int hab_conv2d_fwd(const float* x, const float* w_fwd, const float* bias, float* y, int B, int H, int W, int C,
                              int Cout, int KH, int KW, int stride, int pad, int relu, float* ws, size_t ws_floats,
                              hipStream_t stream) {
    if (!x || !w_fwd || !y) return HAB_ERR_ARG;
    return conv_fwd(mk(B, H, W, C, Cout, KH, KW, stride, pad), x, w_fwd, bias, y, relu, ws, ws_floats, stream);
}
extern "C" int hab_obs_conv2d_fwd(const uint8_t* rgb, const float* depth, const int* rows, const float* w_fwd,
                                  const float* bias, float* y, int B, int H, int W, int Cout, int KH, int KW, int stride,
                                  int pad, int relu, float* ws, size_t ws_floats, hipStream_t stream) {
    if ((!rgb && !depth) || !w_fwd || !y) return HAB_ERR_ARG;
    ObsView o = mkobs(rgb, depth, rows, H, W);
    return obs_conv_fwd(mk(B, H, W, o.C, Cout, KH, KW, stride, pad), o, w_fwd, bias, y, relu, ws, ws_floats, stream);
}
extern "C" int hab_obs_conv2d_fwd_form(const uint8_t* rgb, const float* depth, const int* rows, const float* w_fwd,
                                       const float* bias, float* y, int B, int H, int W, int Cout, int KH, int KW, int stride,
                                       int pad, int relu, const float* ws, size_t ws_floats) {
    if ((!rgb && !depth) || !w_fwd || !y) return HAB_ERR_ARG;
    ObsView o = mkobs(rgb, depth, rows, H, W);
    ObsConvFwdProb p;
    const int r = build(p, mk(B, H, W, o.C, Cout, KH, KW, stride, pad), o, w_fwd, bias, y, relu);
    if (r != HAB_OK) return r;
    return choose_obs_fwd(p, ws, ws_floats, nullptr);
}
extern "C" int hab_conv2d_fwd_form(const float* x, const float* w_fwd, const float* bias, float* y, int B, int H, int W, int C, int Cout,
                                   int KH, int KW, int stride, int pad, int relu, const float* ws, size_t ws_floats) {
    (void)ws; (void)ws_floats;  // no form depends on the workspace
    if (!x || !w_fwd || !y) return HAB_ERR_ARG;
    ConvFwdProb p;
    const int r = build(p, mk(B, H, W, C, Cout, KH, KW, stride, pad), x, w_fwd, bias, y, relu);
    if (r != HAB_OK) return r;
    return choose_conv_fwd(p);
}
extern "C" int hab_conv2d_dgrad(const float* dy, const float* w_dgrad, const float* relu_mask, const float* add, float* dx,
                                int B, int H, int W, int C, int Cout, int KH, int KW, int stride, int pad, float* ws,
                                size_t ws_floats, hipStream_t stream) {
    if (!dy || !w_dgrad || !dx) return HAB_ERR_ARG;
    return conv_dgrad(mk(B, H, W, C, Cout, KH, KW, stride, pad), dy, w_dgrad, relu_mask, add, dx, ws, ws_floats, stream);
}
extern "C" int hab_conv2d_dgrad_form(const float* dy, const float* w_dgrad, const float* relu_mask, const float* add, float* dx,
                                     int B, int H, int W, int C, int Cout, int KH, int KW, int stride, int pad, const float* ws,
                                     size_t ws_floats) {
    (void)ws; (void)ws_floats;  // no form depends on the workspace
    if (!dy || !w_dgrad || !dx) return HAB_ERR_ARG;
    const ConvDesc d = mk(B, H, W, C, Cout, KH, KW, stride, pad);
    const int r = check_conv(d);
    if (r != HAB_OK) return r;
    return choose_conv_dgrad(d, dy, w_dgrad, relu_mask, add, dx);
}
extern "C" int hab_conv2d_wgrad(const float* x, const float* dy, float* dw_oihw, float* dbias, int B, int H, int W, int C, int Cout,
                                int KH, int KW, int stride, int pad, float* ws, size_t ws_floats, hipStream_t stream) {
    if (!x || !dy || !dw_oihw) return HAB_ERR_ARG;
    return conv_wgrad(mk(B, H, W, C, Cout, KH, KW, stride, pad), x, dy, dw_oihw, dbias, ws, ws_floats, stream);
}
extern "C" int hab_obs_conv2d_wgrad(const uint8_t* rgb, const float* depth, const int* rows, const float* dy, float* dw_oihw,
                                    float* dbias, int B, int H, int W, int Cout, int KH, int KW, int stride, int pad, float* ws,
                                    size_t ws_floats, hipStream_t stream) {
    if ((!rgb && !depth) || !dy || !dw_oihw) return HAB_ERR_ARG;
    ObsView o = mkobs(rgb, depth, rows, H, W);
    return obs_conv_wgrad(mk(B, H, W, o.C, Cout, KH, KW, stride, pad), o, dy, dw_oihw, dbias, ws, ws_floats, stream);
}
extern "C" int hab_obs_conv2d_wgrad_form(const uint8_t* rgb, const float* depth, const int* rows, const float* dy, float* dw_oihw,
                                         float* dbias, int B, int H, int W, int Cout, int KH, int KW, int stride, int pad, const float* ws,
                                         size_t ws_floats) {
    if ((!rgb && !depth) || !dy || !dw_oihw) return HAB_ERR_ARG;
    ObsView o = mkobs(rgb, depth, rows, H, W);
    ObsConvWgradProb p;
    const int r = build(p, mk(B, H, W, o.C, Cout, KH, KW, stride, pad), o, dy, dw_oihw, dbias);
    if (r != HAB_OK) return r;
    return choose_obs_wgrad(p, ws, ws_floats);
}
extern "C" int hab_linear_fwd(const float* x, int ldx, const float* w, int ldw, const float* bias, float* y, int ldy, int M,
                              int N, int K, int relu, int accumulate, float* ws, size_t ws_floats, hipStream_t stream) {
    return linear_fwd(x, ldx, w, ldw, bias, y, ldy, M, N, K, relu, accumulate, ws, ws_floats, stream);
}
extern "C" int hab_linear_dgrad(const float* dy, int lddy, const float* w, int ldw, const float* relu_mask, int ldmask,
                                float* dx, int lddx, int M, int n_in, int n_out, int accumulate, float* ws, size_t ws_floats,
                                hipStream_t stream) {
    return linear_dgrad(dy, lddy, w, ldw, relu_mask, ldmask, n_in, dx, lddx, M, n_in, n_out, accumulate, ws, ws_floats, stream);
}
extern "C" int hab_linear_wgrad(const float* dy, int lddy, const float* x, int ldx, float* dw, int lddw, int M, int n_out,
                                int n_in, int perm_c, int perm_hw, int accumulate, float* ws, size_t ws_floats,
                                hipStream_t stream) {
    return linear_wgrad(dy, lddy, x, ldx, dw, lddw, M, n_out, n_in, perm_c, perm_hw, accumulate, ws, ws_floats, stream);
}
extern "C" int hab_debug_dense_trace(long long* out320) {  // development: see dn_trace (dense_bf3.h)
    return (int)hipMemcpyFromSymbol(out320, HIP_SYMBOL(hab::dn_trace), sizeof(long long) * 8 * 8 * 5);
}
extern "C" int hab_colsum(const float* a, int lda, int M, int N, float* out, int accumulate, float* ws, size_t ws_floats,
                          hipStream_t stream) {
    return colsum(a, lda, M, N, out, accumulate, ws, ws_floats, stream);
}
extern "C" int hab_repack_conv_weight(const float* w_oihw, float* w_fwd, float* w_dgrad, int Cout, int Cin, int KH, int KW,
                                      int cin_padded, hipStream_t stream) {
    return repack_conv(w_oihw, w_fwd, w_dgrad, Cout, Cin, KH, KW, cin_padded, stream);
}
extern "C" int hab_repack_flatten_weight(const float* w, float* w_packed, int N, int C, int HW, hipStream_t stream) {
    return repack_flatten(w, w_packed, N, C, HW, stream);
}
extern "C" int hab_transpose2d(const float* w, float* wt, int R, int C, hipStream_t stream) {
    return transpose2d(w, wt, R, C, stream);
}
