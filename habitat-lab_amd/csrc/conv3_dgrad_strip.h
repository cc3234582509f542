// conv3_dgrad_strip.h -- data gradient of SimpleCNN's third convolution (3x3 / stride 1 / no padding, 64 -> 32 channels; 30 x 30 <- 28 x 28
// at 256^2 observations, any height and any width up to 32 through the runtime-geometry instantiation) with the dY STRIP resident in LDS
// and the FILTER slices resident in registers: the scheme of conv2_dgrad_strip.h.
//
//      dX[h][w][ci] = (a2[h][w][ci] > 0) * sum over kh, kw in {0, 1, 2}, co of  dY[h - kh][w - kw][co] * Wd[ci][kh][kw][co]
//      (dY outside Ho x Wo counts as zero; a2 = the convolution's input = conv2's ReLU output)
//
// The ARITHMETIC is that of igemm_bf3_kernel<ConvDgradProb, 1, 2, 4, 1> without split-K, which this kernel replaces, so the results are
// bitwise equal to it wherever that kernel runs unsplit (>= 256 tiles of 128 pixels): per output value ONE accumulation chain over the 18
// k-steps (k-step s = 2 tap + co half, tap = 3 kh + kw) with the six plane products of a k-step in the same order, and the same sign
// schedule -- pixel m = (img H + h) W + w accumulates the negated sum when (m >> 7) & 1.
//
//   * a workgroup owns R output rows of one frame: the R + 2 dY rows are read from HBM once, split once, stored [pixel][32 channels] as
//     three bf16 planes (64-byte pixel rows, 34 pixel columns: two zero columns left, at least two right; zero rows outside the image),
//     16-byte chunks XOR-swizzled by (pixel >> 2) & 3: the 16 lanes of a ds_read_b128 group read consecutive pixels in runs of 4 and 8
//     whose quads (pixel >> 2) differ mod 4 wherever pixel & 3 agrees, so a group covers all 64 banks whatever the first pixel.  A second
//     copy of the three planes holds the negated values: a lane reads the copy its output pixel's sign asks for (the copies are a
//     multiple of 256 bytes apart, so the banks do not change);
//   * one output row is one 32-pixel MFMA tile (columns >= W are computed and not stored), N = 64 input channels in two halves;
//   * wave w of 8: output row w & 1 of a row pair, channel half (w >> 1) & 1, k-steps [9 z, 9 z + 9) with z = w >> 2.  Its filter slice
//     -- 9 k-steps x 3 planes = 108 VGPRs -- stays in registers; per output row it reads 27 fragments and issues 54 MFMAs (operands
//     swapped: a lane ends up with 4 consecutive input channels of one output pixel);
//   * the chain is handed on, not summed: the z = 0 wave starts row pair p from zero and leaves its accumulator in LDS, the z = 1 wave
//     takes it as the start of its own nine k-steps one phase later (while z = 0 works on pair p + 1), applies the ReLU mask and stores
//     from registers, 16 bytes per lane.  R / 2 + 1 phases per item, one barrier each.
#pragma once
#include "igemm_bf3.h"
#include "ops.h"

#include <atomic>

namespace hab {

struct C3dArgs {
    const float* dy;    // [B][Ho][Wo][32]
    const float* wd;    // packed filter [64 ci][3][3][32 co] (the engine's data-gradient layout)
    const float* mask;  // [B][H][W][64] or null: dX *= (mask > 0)
    float* dx;          // [B][H][W][64]
    int B;
    int strips, items;
    int sign_schedule;
    int H, W, Ho, Wo;   // runtime-geometry instantiation (RT): dX is H x W (W <= 32), dY is Ho x Wo
    unsigned* ctr;      // 8 per-XCD draw counters + a leave counter (a slot of c3d_draw_pool)
};

// Item order: the workgroups of an XCD draw the next item of THEIR XCD's run from a counter, as conv_patch_bf3_kernel does -- a workgroup
// that starts late (more than 128 VGPRs: it does not fit beside the persistent recurrence of the second stream, which holds 32 CUs for
// the length of a time chunk) simply takes fewer items instead of holding the kernel's tail.  Counters: a small pool of device slots, zero
// at load, zeroed again by the last workgroup of the launch that used them -- no memset on the stream; launches in flight at once get
// different slots.  An item's arithmetic does not depend on who computes it.
constexpr int C3D_DRAW_SLOTS = 64;
__device__ unsigned c3d_draw_pool[C3D_DRAW_SLOTS * 16];

template <int R>
struct C3dCfg {
    static constexpr int H = 30, Ho = 28, Wo = 28, NT = 512, MAXWO = 30;
    static constexpr int YRS = R + 2, YCOLS = 34, YPIX = YRS * YCOLS;
    static constexpr int YU = YRS * Wo * 8, YPT = (YRS * MAXWO * 8 + NT - 1) / NT;   // staging units: 4 channels of one dY pixel
    static constexpr int Y_PLANE = YPIX * 32;                                       // bf16 elements
    static constexpr int Y_COPY = 3 * Y_PLANE;                                      // bf16 elements: the negated copy follows the plain one
    static constexpr size_t Y_BYTES = (size_t)2 * Y_COPY * 2, PASS_BYTES = (size_t)2 * 4 * 16 * 64 * 4;  // hand-over: two buffers, taken in turn
    static constexpr size_t LDS_BYTES = Y_BYTES + PASS_BYTES;
    static_assert(R % 2 == 0, "the waves take the rows of a strip in pairs");
    static_assert((Y_COPY * 2) % 256 == 0, "both copies on the same banks");
};

// RT = false: the benchmark geometry, every index a compile-time constant; RT = true: H, W, Ho, Wo from the arguments (W <= 32: one
// 32-pixel tile per row, the LDS image keeps its 34 pixel columns -- the columns beyond Wo + 2 stay zero).
template <int R, bool RT>
__global__ void __launch_bounds__(512) conv3_dgrad_strip_kernel(const C3dArgs a) {
    using Cfg = C3dCfg<R>;
    constexpr int NT = Cfg::NT;
    const int H = RT ? a.H : Cfg::H, W = RT ? a.W : Cfg::H, Ho = RT ? a.Ho : Cfg::Ho, Wo = RT ? a.Wo : Cfg::Wo;
    const int YU = Cfg::YRS * Wo * 8;
    extern __shared__ __attribute__((aligned(16))) unsigned short smem16[];
    unsigned short* ys = smem16;                                                             // [copy][plane][YPIX][32], swizzled
    f32x4* pass = reinterpret_cast<f32x4*>(reinterpret_cast<char*>(smem16) + Cfg::Y_BYTES);   // [2][4 waves][4 quads][64 lanes]
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int rsel = wave & 1, chalf = (wave >> 1) & 1, z = wave >> 2;
    const int li = lane & 31, hi = lane >> 5;

    // this XCD's run of items: [run0, run0 + run_len); s_draw: the draws for the first two items, then the one for the item after next
    __shared__ int s_draw[2];
    const int xcd = blockIdx.x & 7;
    const int per_xcd = (a.items + 7) >> 3, run0 = xcd * per_xcd, run_len = max(0, min(a.items, run0 + per_xcd) - run0);
    if (t == 0) { s_draw[0] = (int)atomicAdd(a.ctr + xcd, 1u); s_draw[1] = (int)atomicAdd(a.ctr + xcd, 1u); }

    // border columns (and everything else until staged) read as zero
    for (int i = t; i < (int)(Cfg::Y_BYTES / 16); i += NT) reinterpret_cast<u32x4*>(smem16)[i] = u32x4{0u, 0u, 0u, 0u};

    // ---- this wave's filter slice: k-step 9 z + j = (tap, 16 output channels); lane = (input channel li of the half, 8 output channels) ----
    bf16x8 bw[9][3];
    int tapoff[9];  // LDS pixel offset of the tap, relative to the output pixel's own position in the image: (2 - kh) rows, (2 - kw) columns
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int s = 9 * z + j, tap = s >> 1, coh = s & 1, kh = tap / 3, kw = tap - 3 * kh;
        tapoff[j] = (2 - kh) * Cfg::YCOLS + 2 - kw;
        const float* src = a.wd + ((size_t)(chalf * 32 + li) * 9 + tap) * 32 + coh * 16 + hi * 8;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
        const Bf3Planes sp = bf3_split8(v0, v1, 0u);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) bw[j][pl] = sp.p[pl];
    }

    f32x4 yr[Cfg::YPT];
    int pf_h0 = 0;  // first output row of the strip whose loads are in yr
    auto fetch = [&](int item) {  // issues the loads only; rows outside the image load the tensor's first bytes (zeroed at stage)
        const int img = item / a.strips, h0 = (item - img * a.strips) * R;
        pf_h0 = h0;
#pragma unroll
        for (int j = 0; j < Cfg::YPT; ++j) {
            const int u = t + j * NT;
            const int r = u / (Wo * 8), row = h0 - 2 + r;
            const bool ok = u < YU && (unsigned)row < (unsigned)Ho;
            const size_t off = ok ? ((size_t)img * Ho + row) * (size_t)(Wo * 32) + (size_t)(u - r * (Wo * 8)) * 4 : 0;
            yr[j] = *reinterpret_cast<const f32x4*>(a.dy + off);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < Cfg::YPT; ++j) {
            const int u = t + j * NT;
            if (u >= YU) continue;
            const int r = u / (Wo * 8), rem = u - r * (Wo * 8), w = rem >> 3, c4 = rem & 7;
            const int pixidx = r * Cfg::YCOLS + w + 2;
            unsigned short* dst = ys + pixidx * 32 + (((c4 >> 1) ^ ((pixidx >> 2) & 3)) << 3) + (c4 & 1) * 4;
            const bool in_image = (unsigned)(pf_h0 - 2 + r) < (unsigned)Ho;
            const f32x4 v = in_image ? yr[j] : f32x4{0.f, 0.f, 0.f, 0.f};
            unsigned w0[3], w1[3];
            bf3_split2(v[0], v[1], w0[0], w0[1], w0[2]);
            bf3_split2(v[2], v[3], w1[0], w1[1], w1[2]);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {  // the split of -x is the negated split of x: rounding to nearest is symmetric
                *reinterpret_cast<u32x2*>(dst + pl * Cfg::Y_PLANE) = u32x2{w0[pl], w1[pl]};
                *reinterpret_cast<u32x2*>(dst + Cfg::Y_COPY + pl * Cfg::Y_PLANE) = u32x2{w0[pl] ^ 0x80008000u, w1[pl] ^ 0x80008000u};
            }
        }
    };

    __syncthreads();  // the zero fill is complete, the first draws are visible
    int cur = s_draw[0], nxt = s_draw[1];
    if (cur < run_len) fetch(run0 + cur);
    for (int it = 0; cur < run_len; ++it) {
        const int item = run0 + cur;
        stage();
        __syncthreads();
        const bool more = nxt < run_len;
        if (more) fetch(run0 + nxt);
        // the draw for the item after next: written now, read behind this item's barriers (two slots: the other one was read at the end
        // of the previous item, an item of barriers ago)
        if (more && t == 0) s_draw[it & 1] = (int)atomicAdd(a.ctr + xcd, 1u);
        const int img = item / a.strips, h0 = (item - img * a.strips) * R;
#pragma unroll 1
        for (int ph = 0; ph <= R / 2; ++ph) {  // phase ph: the z = 0 waves on row pair ph, the z = 1 waves on row pair ph - 1
            const int rp = ph - z;
            if (rp >= 0 && rp < R / 2) {  // wave-uniform
                const int tr = 2 * rp + rsel, h = h0 + tr;
                const bool live = h < H && li < W;
                const size_t out = (((size_t)img * H + h) * W + li) * 64 + chalf * 32 + 4 * hi;  // + 8 g: this lane's value quad g
                const bool flip = a.sign_schedule && ((((img * H + h) * W + li) >> 7) & 1);       // the replaced kernel's 128-pixel tiles
                // ReLU-mask quads of this row, requested BEFORE its MFMAs
                f32x4 mk[4];
                if (z == 1 && a.mask) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) mk[g] = *reinterpret_cast<const f32x4*>(a.mask + (live ? out + 8 * g : (size_t)0));
                }
                // dY pixel of output pixel li of strip row tr under tap (kh, kw): LDS row tr + 2 - kh, column li + 2 - kw
                const int pix0 = tr * Cfg::YCOLS + li;
                const unsigned short* ysl = ys + (flip ? Cfg::Y_COPY : 0);
                f32x4* hand = pass + (size_t)((((ph - z) & 1) * 4 + (wave & 3)) * 4) * 64 + lane;  // z = 0 writes buffer ph & 1, z = 1 reads it one phase later
                f32x16 acc;
                if (z == 0) {
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 q = hand[g * 64];
                        acc[4 * g] = q[0]; acc[4 * g + 1] = q[1]; acc[4 * g + 2] = q[2]; acc[4 * g + 3] = q[3];
                    }
                }
                // the fragments of k-step j + 1 are requested before the MFMAs of k-step j (left to itself the compiler reads just in
                // time and every k-step waits out the LDS latency); the scheduling barrier keeps the reads where they are written
                bf16x8 yf[2][3];
                auto read_frags = [&](int j, bf16x8* f) {
                    const int pixidx = pix0 + tapoff[j];
                    const int chunk = 2 * ((9 * z + j) & 1) + hi;
                    const unsigned short* src = ysl + pixidx * 32 + ((chunk ^ ((pixidx >> 2) & 3)) << 3);
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) f[pl] = *reinterpret_cast<const bf16x8*>(src + pl * Cfg::Y_PLANE);
                };
                read_frags(0, yf[0]);
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    if (j + 1 < 9) read_frags(j + 1, yf[(j + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                    // A: dY, B: filter
#pragma unroll
                    for (int q = 0; q < 6; ++q)  // operands swapped: D[m = input channel][n = pixel]
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[j][BF3_PB[q]], yf[j & 1][BF3_PA[q]], acc, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (z == 0) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) hand[g * 64] = f32x4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
                } else if (live) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f32x4 s = f32x4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
                        if (flip) s = -s;
                        if (a.mask) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) s[e] = mk[g][e] > 0.f ? s[e] : 0.f;
                        }
                        *reinterpret_cast<f32x4*>(a.dx + out + 8 * g) = s;
                    }
                }
            }
            __syncthreads();  // the hand-over of this phase is written; after the last phase: every wave is done with this strip's image
        }
        cur = nxt;
        nxt = more ? s_draw[it & 1] : run_len;
    }
    // the last workgroup to leave zeroes the counters for the next launch that is handed this slot
    if (t == 0) {
        __threadfence();
        if (atomicAdd(a.ctr + 8, 1u) == gridDim.x - 1) {
#pragma unroll
            for (int i = 0; i < 9; ++i) a.ctr[i] = 0u;
        }
    }
}

inline bool conv3_dgrad_strip_covers(const ConvDesc& d) {
    return d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 0 && d.C == 64 && d.Cout == 32 && d.H >= 3 && d.W >= 3 && d.W <= 32;
}
constexpr int C3D_ROWS = 6;  // output rows per strip: 5 strips per 30-row frame
// the form serves this call (host only: the dispatch rule and the launcher both ask it)
inline bool conv3_dgrad_strip_serves(const ConvDesc& d, const float* dy, const float* wd, const float* mask, const float* add, const float* dx) {
    if (!conv3_dgrad_strip_covers(d)) return false;
    if (add || d.B < 16 || !dy || !wd || !dx) return false;
    if ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(wd) | reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(mask)) & 15) return false;
    if ((long long)d.B * d.H * d.W > 0x7fffffffLL) return false;  // pixel indices are ints
    return (long long)d.B * cdiv(d.H, C3D_ROWS) <= 0x7fffffffLL;
}

// HAB_NOT_APPLICABLE: call not served.
inline int conv3_dgrad_strip(const ConvDesc& d, const float* dy, const float* wd, const float* mask, const float* add, float* dx,
                             hipStream_t stream) {
    if (!conv3_dgrad_strip_serves(d, dy, wd, mask, add, dx)) return HAB_NOT_APPLICABLE;
    constexpr int R = C3D_ROWS;
    using Cfg = C3dCfg<R>;
    C3dArgs a;
    a.dy = dy; a.wd = wd; a.mask = mask; a.dx = dx; a.B = d.B;
    a.H = d.H; a.W = d.W; a.Ho = d.H - 2; a.Wo = d.W - 2;
    a.strips = cdiv(d.H, R);
    a.items = d.B * a.strips;
    a.sign_schedule = bf3_sign_schedule();
    static std::atomic<unsigned> next_slot{0};
    static unsigned* pool = nullptr;
    static const hipError_t sym_err = hipGetSymbolAddress(reinterpret_cast<void**>(&pool), HIP_SYMBOL(c3d_draw_pool));
    if (sym_err != hipSuccess || !pool) return HAB_ERR_ARG;
    a.ctr = pool + (size_t)(next_slot.fetch_add(1, std::memory_order_relaxed) % C3D_DRAW_SLOTS) * 16;
    const int grid = persistent_grid(a.items);
    if (d.H == Cfg::H && d.W == Cfg::H) {
        HAB_TRY((lds_opt_in<conv3_dgrad_strip_kernel<R, false>>((int)Cfg::LDS_BYTES)));
        conv3_dgrad_strip_kernel<R, false><<<grid, Cfg::NT, Cfg::LDS_BYTES, stream>>>(a);
    } else {
        HAB_TRY((lds_opt_in<conv3_dgrad_strip_kernel<R, true>>((int)Cfg::LDS_BYTES)));
        conv3_dgrad_strip_kernel<R, true><<<grid, Cfg::NT, Cfg::LDS_BYTES, stream>>>(a);
    }
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

}  // namespace hab
