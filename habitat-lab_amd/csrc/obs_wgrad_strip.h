// obs_wgrad_strip.h -- weight gradient of SimpleCNN's first convolution (8x8 / stride 4, RGB-D -> Cout <= 32) with the observation rows
// under a tile resident in LDS.  Same arithmetic as obs_wgrad_bf3.h, bit for bit; only the way the operands reach the MFMA differs.
//
// obs_wgrad_bf3.h gathers im2col rows: every observation element is fetched and converted four times (2x from the kw overlap inside
// a tile, 2x from the kh overlap of consecutive output rows) and both operands are transposed in registers -- 11 VALU instructions per
// MFMA.  Here, as in stem_wgrad_strip.h and wgrad3x3_bf3.h:
//   * the 8 input rows under an output row live in a ring of 8 LDS row slots (input row a in slot a & 7), rgb as [slot][W][3] bf16 (one
//     plane: a uint8 is exact in bf16) and depth as three planes [slot][W] of the exact 3-term split.  Rows are read from HBM whole, 12 B
//     of rgb + 16 B of depth per thread and unit of 4 pixels, and converted once.  Consecutive tiles of a workgroup are consecutive output
//     rows of one frame: 4 of their 8 rows stay, so a tile loads 4 rows, all 8 when its run begins or the frame changes, none for the
//     second 64-pixel block of a wide row;
//   * dY is stored pixel-major as loaded, [pixel][32 channels] in three planes, one bf3_store4 per loaded f32x4;
//   * fragments are built by the LDS transpose read (bf3_tr_read, bf3_split.h): a 16-lane group passes the chunks (pixel p, 4 consecutive
//     reduction slots) of four pixels and receives the k-contiguous fragment.  For rgb the slot inside a filter row is m = kw * 3 + c:
//     the 24 slots of output pixel wo are the 24 consecutive elements at column 4 wo of the row, so a chunk of 4 never leaves its filter
//     row and is 8-byte aligned (pixel pitch 24 B).  For depth the slot is kw (pixel pitch 8 B).  No register transposes.
// Tile partition, k-groups of the four waves, accumulators, product order, sign schedule, cross-wave fold, epilogue and split-K pass
// are those of obs_wgrad_bf3.h, and the operand values are the same bf16 patterns: dW and db come out bitwise equal for the same
// arguments and workspace size (tests/test_gpu_obs_wgrad_strip.py).  A pixel beyond Wo reads the row's last pixel (as the im2col gather
// does) against dY = 0.
//
// LDS banking of the transpose reads (bank = (byte / 4) % 64 per 32-lane half): dY -- 4 pixels x 64 B contiguous; depth -- per filter
// row 5 chunks of 8 B, the 4 rows of a half 64 B apart modulo 256 (row pitch = 64 mod 256); rgb -- the 32 slots of a half lie in at most
// two filter rows, <= 120 B each, 128 B apart modulo 256 (row pitch = 128 mod 256).  Equal addresses are one access.
#pragma once
#include "obs_wgrad_bf3.h"

namespace hab {

constexpr int OWS_MAXU = 4;              // staging units (4 pixels of one row) per thread when all 8 rows load, at most: W <= 512
constexpr int OWS_YP = OWG_BK * 32;      // bf16 elements per dY plane
constexpr size_t OWS_RED_BYTES = 256 * 32 * sizeof(float);  // the cross-wave fold's buffer

struct ObsWgradStripGeom {
    FastDiv dUPR;
    int UPR;     // staging units per input row: W / 4
    int RP, DP;  // LDS row pitch of the rgb / depth rows, bf16 elements
};

// MAXU: staging units per thread when all 8 rows load, 8 * (W / 4) <= 256 MAXU
template <int MAXU>
__global__ void __launch_bounds__(256, 2) obs_wgrad_bf3_kernel_strip(const ObsConvWgradProb p, const ObsWgradGeom gg, const ObsWgradStripGeom sg,
                                                                     float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned short smem16[];
    const int RP = sg.RP, DP = sg.DP, DPL = 8 * sg.DP;
    unsigned short* Rs = smem16;           // [8][RP]         element (column w, channel c) of a row at w * 3 + c
    unsigned short* Ds = Rs + 8 * RP;      // [3][8][DP]
    unsigned short* Ys = Ds + 3 * DPL;     // [3][64][32]     [pixel of the tile][co]

    const int t = threadIdx.x;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int li = lane & 31, hi = lane >> 5;
    const ConvGeom& g = p.g;

    // dY staging role: channels 4 coq .. +3 of the pixel pair 2 kr, 2 kr + 1 (the pair obs_wgrad_bf3.h's role coq * 32 + kr sums for the
    // bias gradient); odd kr take the odd pixel first, so that the 8-byte LDS stores of 32 lanes cover 128 contiguous bytes twice over
    const int b_coq = t & 7, b_kr = t >> 3;
    const int b_role = b_coq * 32 + b_kr;
    const bool b_col_ok = b_coq * 4 < p.N;  // N % 4 == 0 (checked by the launcher)

    const int tile_begin = blockIdx.x * gg.tiles_per_wg;
    const int tile_end = min(gg.tiles, tile_begin + gg.tiles_per_wg);

    struct Rgb12 { uint32_t d0, d1, d2; };
    Rgb12 x_rgb[MAXU];
    f32x4 x_dep[MAXU], b_raw[2];
    int u_row[MAXU], u_col[MAXU];  // unit t + 256 j of a load: row, and unit inside the row
#pragma unroll
    for (int j = 0; j < MAXU; ++j) sg.dUPR.divmod(t + j * 256, u_row[j], u_col[j]);
    f32x4 cs = zero4();
    const bool has_cs = p.colsum != nullptr;
    int res_img = -1, res_ho = 0;  // the output row whose 8 input rows are resident, or on their way
    int pf_a0 = 0, pf_n = 0;       // input rows pf_a0 .. pf_a0 + pf_n - 1 of that frame are in x_rgb / x_dep

    auto fetch = [&](int tile) {
        int row, wb, img, ho;
        gg.dWB.divmod(tile, row, wb);
        gg.dHo.divmod(row, img, ho);
        const bool same = img == res_img && ho == res_ho, next = img == res_img && ho == res_ho + 1;
        pf_n = same ? 0 : (next ? 4 : 8);
        pf_a0 = ho * 4 + 8 - pf_n;
        res_img = img; res_ho = ho;
        if (pf_n) {
            const int srow = p.obs.srow(img);
            const size_t fpix = ((size_t)srow * g.H + pf_a0) * g.W;  // rows are contiguous: unit u is pixels 4 u .. 4 u + 3 from here
            const uint8_t* rgb = p.obs.rgb + fpix * 3;               // block-uniform bases, 32-bit lane offsets (8 rows < 2^31 bytes)
            const float* dep = p.obs.depth + fpix;
            const int nunits = pf_n * sg.UPR;
#pragma unroll
            for (int j = 0; j < MAXU; ++j) {
                const unsigned u = t + j * 256;
                if (u < (unsigned)nunits) {
                    x_rgb[j] = *reinterpret_cast<const Rgb12*>(rgb + u * 12u);
                    x_dep[j] = ld4(dep + u * 4u);
                }
            }
        }
        const float* dyrow = p.dy + ((size_t)row * g.Wo) * p.N;  // block-uniform; one output row is < 2^31 bytes
        const int wq = wb * OWG_BK + b_kr * 2;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int wo = wq + (r ^ (b_kr & 1));
            const bool ok = b_col_ok & (wo < g.Wo);
            b_raw[r] = ok ? ld4(dyrow + (unsigned)(wo * p.N + b_coq * 4)) : zero4();
        }
    };
    auto stage = [&]() {
        const int nunits = pf_n * sg.UPR;
#pragma unroll
        for (int j = 0; j < MAXU; ++j) {
            if (t + j * 256 < nunits) {
                const int c = u_col[j], slot = (pf_a0 + u_row[j]) & 7;
                // rgb: byte i of the 12 is element i of the 4 pixels x 3 channels
                unsigned f[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) {
                    const unsigned d = (i >> 2) == 0 ? x_rgb[j].d0 : ((i >> 2) == 1 ? x_rgb[j].d1 : x_rgb[j].d2);
                    f[i] = __float_as_uint((float)((d >> (8 * (i & 3))) & 0xffu));  // exact in bf16
                }
                unsigned short* dr = Rs + slot * RP + c * 12;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    u32x2 wv;
                    wv[0] = bf3_pack(f[4 * q], f[4 * q + 1]);
                    wv[1] = bf3_pack(f[4 * q + 2], f[4 * q + 3]);
                    *reinterpret_cast<u32x2*>(dr + 4 * q) = wv;
                }
                unsigned short* dd = Ds + slot * DP + c * 4;
                bf3_store4(x_dep[j], dd, dd + DPL, dd + 2 * DPL);
            }
        }
        if (has_cs) cs += b_raw[0] + b_raw[1];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            unsigned short* d = Ys + (b_kr * 2 + (r ^ (b_kr & 1))) * 32 + b_coq * 4;
            bf3_store4(b_raw[r], d, d + OWS_YP, d + 2 * OWS_YP);
        }
    };

    // Lane constants of the transpose reads.  16-lane group g16 = (lane >> 4) & 1 serves rows 16 g16 .. + 15 of a 32-row operand tile,
    // k-block hi = lane >> 5; lane i of a group passes the chunk of pixel p4 = i >> 2 of the group's four and of chunk q4 = i & 3.
    const int i16 = lane & 15, g16 = (lane >> 4) & 1, p4 = i16 >> 2, q4 = i16 & 3;
    const int ychunk = (wave * 16 + hi * 8 + p4) * 32 + g16 * 16 + q4 * 4;
    // rgb tile mt: reduction rows R0 .. R0 + 3 with R0 = 32 mt + 16 g16 + 4 q4 = 24 kh + m0
    int rgb_off[6], rgb_hi[6];
#pragma unroll
    for (int mt = 0; mt < 6; ++mt) {
        const int R0 = 32 * mt + 16 * g16 + 4 * q4, kh = R0 / 24;
        rgb_off[mt] = (kh & 3) * RP + (R0 - 24 * kh);
        rgb_hi[mt] = kh >> 2;
    }
    // depth tile dt: taps 32 dt + 16 g16 + 4 q4 .. + 3 = filter row 4 dt + 2 g16 + (q4 >> 1), kw0 = 4 (q4 & 1)
    const int dep_off = (2 * g16 + (q4 >> 1)) * DP + 4 * (q4 & 1);

    f32x16 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[i][v] = 0.0f;

    // sign schedule of obs_wgrad_bf3.h: waves 2, 3 accumulate the negated sum (dY fragments sign-flipped as they are read)
    const unsigned sf = wave >= 2 ? 0x80008000u : 0u;
    u32x4 sign_flip;
    sign_flip[0] = sf; sign_flip[1] = sf; sign_flip[2] = sf; sign_flip[3] = sf;
    if (tile_begin < tile_end) fetch(tile_begin);
    for (int tile = tile_begin; tile < tile_end; ++tile) {
        stage();
        __syncthreads();
        if (tile + 1 < tile_end) fetch(tile + 1);
        int row, wb, img, ho;
        gg.dWB.divmod(tile, row, wb);
        gg.dHo.divmod(row, img, ho);
        // filter rows 0 .. 3 are input rows 4 ho .. + 3 = slots 4 (ho & 1) .., filter rows 4 .. 7 the other half of the ring
        const int half[2] = {(ho & 1) * 4, 4 - (ho & 1) * 4};
        const int wo_lane = wb * OWG_BK + wave * 16 + hi * 8 + p4;
        const int wo0 = min(wo_lane, g.Wo - 1), wo1 = min(wo_lane + 4, g.Wo - 1);
        bf16x8 b[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            u32x4 raw = __builtin_bit_cast(u32x4, bf3_join(bf3_tr_read(Ys + pl * OWS_YP + ychunk), bf3_tr_read(Ys + pl * OWS_YP + ychunk + 4 * 32)));
            raw ^= sign_flip;
            b[pl] = __builtin_bit_cast(bf16x8, raw);
        }
#pragma unroll
        for (int mt = 0; mt < 6; ++mt) {
            const unsigned short* ar = Rs + (rgb_hi[mt] ? half[1] : half[0]) * RP + rgb_off[mt];
            const bf16x8 a = bf3_join(bf3_tr_read(ar + wo0 * 12), bf3_tr_read(ar + wo1 * 12));
#pragma unroll
            for (int pl = 2; pl >= 0; --pl) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[pl], acc[mt], 0, 0, 0);
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            const unsigned short* ad = Ds + half[dt] * DP + dep_off;
            bf16x8 a[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                a[pl] = bf3_join(bf3_tr_read(ad + pl * DPL + wo0 * 4), bf3_tr_read(ad + pl * DPL + wo1 * 4));
#pragma unroll
            for (int q = 0; q < 6; ++q) acc[6 + dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[BF3_PA[q]], b[BF3_PB[q]], acc[6 + dt], 0, 0, 0);
        }
        __syncthreads();  // every wave is done with this tile's dY and with the 4 row slots the next tile replaces
    }

    // ---- sum the four waves (k-groups) through LDS, then write this workgroup's slab in the problem's row order i = tap*4 + ci ----
    float* red = reinterpret_cast<float*>(smem16);  // [256][32] fp32 = 32 KB (the tile buffers are free: last barrier passed)
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int mt = 0; mt < 8; ++mt)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int rrow = mt * 32 + (v & 3) + 8 * (v >> 2) + 4 * hi;
                    float* dst = red + rrow * 32 + li;
                    *dst = (w == 0 ? 0.f : *dst) + (w >= 2 ? -acc[mt][v] : acc[mt][v]);
                }
        }
        __syncthreads();
    }
    const int MP = p.M + (has_cs ? 1 : 0);
    float* slab = partial + (size_t)blockIdx.x * MP * p.N;
    for (int e = t; e < 256 * 32; e += 256) {
        const int rrow = e >> 5, co = e & 31;
        const int i = rrow < OWG_RGB_ROWS ? (rrow / 3) * 4 + (rrow % 3) : (rrow - OWG_RGB_ROWS) * 4 + 3;
        if (co < p.N) slab[(size_t)i * p.N + co] = red[e];
    }
    if (has_cs) {  // bias gradient: column sums of dY; role coq * 32 + kr holds channels coq*4.. of its pixel pairs
        __syncthreads();
        *reinterpret_cast<f32x4*>(red + b_role * 4) = cs;
        __syncthreads();
        if (t < p.N) {
            float s = 0.f;
            for (int q = 0; q < 32; ++q) s += red[((t >> 2) * 32 + q) * 4 + (t & 3)];
            slab[(size_t)p.M * p.N + t] = s;
        }
    }
}

// The geometry this form covers, on top of obs_wgrad_bf3_covers: the 8x8 / stride 4 filter and rows of at most 512 pixels.
inline bool obs_wgrad_strip_covers(const ObsConvWgradProb& p, const float* ws, size_t ws_floats) {
    const ConvGeom& g = p.g;
    return obs_wgrad_bf3_covers(p, ws, ws_floats) && g.KH == 8 && g.KW == 8 && g.stride == 4 && 8 * (g.W / 4) <= OWS_MAXU * 256 &&
           (long long)g.Wo * p.N * 4 < (1ll << 31);
}

// returns HAB_OK, an error, or HAB_NOT_APPLICABLE when the problem / workspace does not fit this form (the caller tries obs_wgrad_bf3_launch)
inline int obs_wgrad_strip_launch(const ObsConvWgradProb& p, float* ws, size_t ws_floats, hipStream_t stream) {
    if (!obs_wgrad_strip_covers(p, ws, ws_floats)) return HAB_NOT_APPLICABLE;
    const ConvGeom& g = p.g;
    ObsWgradGeom gg;
    const int wgs = obs_wgrad_partition(p, ws_floats, gg);
    ObsWgradStripGeom sg;
    sg.UPR = g.W / 4;
    sg.dUPR = FastDiv(sg.UPR);
    sg.RP = (((g.W * 6 + 127) / 256) * 256 + 128) / 2;  // >= 3 W elements, 128 B modulo 256
    sg.DP = (((g.W * 2 + 191) / 256) * 256 + 64) / 2;   // >= W elements, 64 B modulo 256
    size_t lds = ((size_t)8 * sg.RP + (size_t)3 * 8 * sg.DP + (size_t)3 * OWS_YP) * 2;
    if (lds < OWS_RED_BYTES) lds = OWS_RED_BYTES;
    if (8 * sg.UPR <= 2 * 256) {  // W <= 256
        obs_wgrad_bf3_kernel_strip<2><<<wgs, 256, lds, stream>>>(p, gg, sg, ws);
    } else {
        HAB_TRY(lds_opt_in<obs_wgrad_bf3_kernel_strip<OWS_MAXU>>(80 * 1024));
        obs_wgrad_bf3_kernel_strip<OWS_MAXU><<<wgs, 256, lds, stream>>>(p, gg, sg, ws);
    }
    HAB_LAUNCH_CHECK();
    igemm_splitk_reduce<ObsConvWgradProb>(p, ws, wgs, stream);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

}  // namespace hab
