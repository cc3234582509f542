// obs_ops.hip -- observation transformers on the device (N4).
//
// Reference: habitat_baselines/common/obs_transformers.py:70-231 (ResizeShortestEdge, CenterCropper) through
// habitat_baselines/utils/common.py:481-557 (image_resize_shortest_edge = F.interpolate(mode "area" | "nearest") on the NCHW
// float view and a cast back to the sensor dtype; center_crop = a slice).  Real ObjectNav sensors are 640x480 and the policy
// wants 256x256: the reference runs permute -> float -> adaptive_avg_pool2d -> cast -> permute -> slice per sensor, six passes
// over HBM and four temporaries.  Here ONE launch reads each source pixel once and writes the cropped, resized NHWC frame
// straight into its destination (a rollout-storage row): only the resized pixels that survive the crop are computed.
//
// Arithmetic is ATen's, so the result is bit-identical to the reference on CPU:
//   area    : window [floor(i*H/h), ceil((i+1)*H/h)) x [floor(j*W/w), ceil((j+1)*W/w)) (integer index math of
//             adaptive_avg_pool2d), fp32 sum in row-major window order, then sum / kh / kw (two divisions, as ATen), then the cast
//             (uint8: truncation);
//   nearest : src = min(int(floorf(dst * float(in) / out)), in - 1)  (upsample_nearest's float scale), plain copy.
// HBM-bound: bytes per frame = source window bytes read once + output bytes written once.
#include <type_traits>

#include "ops.h"
#include "../../include/habitat_amd.h"

namespace hab {

struct ResizeCropArgs {
    const void* src; void* dst;
    int N, H, W, C;        // source NHWC
    int rh, rw;            // extent of the (virtual) resized image
    int y0, x0, oh, ow;    // crop window inside the resized image = output extent
    int mode;              // 0 area, 1 nearest
};

template <class T>
struct PixCast;
template <> struct PixCast<uint8_t> { static __device__ uint8_t from(float v) { return (uint8_t)v; } };
template <> struct PixCast<float>   { static __device__ float from(float v) { return v; } };
template <> struct PixCast<int32_t> { static __device__ int32_t from(float v) { return (int32_t)v; } };

__device__ inline int nearest_src(int dst, int in, int out) {
    if (in == out) return dst;
    if (out == 2 * in) return dst >> 1;
    const float scale = (float)in / (float)out;
    const int s = (int)floorf((float)dst * scale);
    return s < in - 1 ? s : in - 1;
}

#pragma clang fp contract(off)
template <class T, int CMAX>
__global__ void __launch_bounds__(256) obs_resize_crop_kernel(const ResizeCropArgs a) {
    const long long total = (long long)a.N * a.oh * a.ow;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int ox = (int)(e % a.ow);
        long long r = e / a.ow;
        const int oy = (int)(r % a.oh);
        const int n = (int)(r / a.oh);
        const int ry = oy + a.y0, rx = ox + a.x0;
        const T* img = static_cast<const T*>(a.src) + (size_t)n * a.H * a.W * a.C;
        T* out = static_cast<T*>(a.dst) + ((size_t)e) * a.C;
        if (a.mode == 1) {
            const T* p = img + ((size_t)nearest_src(ry, a.H, a.rh) * a.W + nearest_src(rx, a.W, a.rw)) * a.C;
            for (int c = 0; c < a.C; ++c) out[c] = p[c];
            continue;
        }
        // adaptive_avg_pool2d index math: start = floor(i * in / out), end = ceil((i + 1) * in / out)
        const int ys = (int)(((long long)ry * a.H) / a.rh), ye = (int)((((long long)ry + 1) * a.H + a.rh - 1) / a.rh);
        const int xs = (int)(((long long)rx * a.W) / a.rw), xe = (int)((((long long)rx + 1) * a.W + a.rw - 1) / a.rw);
        float sum[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) sum[c] = 0.f;
        for (int y = ys; y < ye; ++y) {
            const T* row = img + ((size_t)y * a.W + xs) * a.C;
            for (int x = xs; x < xe; ++x, row += a.C) {
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (c < a.C) sum[c] = sum[c] + (float)row[c];
            }
        }
        const float kh = (float)(ye - ys), kw = (float)(xe - xs);
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < a.C) out[c] = PixCast<T>::from(__fdiv_rn(__fdiv_rn(sum[c], kh), kw));  // ATen: sum / kh / kw, two IEEE divisions
    }
}

// Area mode, LDS-staged: a workgroup owns an 8 x 32 tile of output pixels of one frame.  The source footprint of the tile (about
// 16 rows x 62 pixels at the 640x480 -> 256 geometry) is copied to LDS with coalesced 32-bit loads (uint8 rgb: 3 loads per thread
// instead of 27 byte loads per output pixel), then every thread sums its window from LDS in ATen's order.
constexpr int RC_TH = 8, RC_TW = 32;
template <class T, int C>
__global__ void __launch_bounds__(256) obs_resize_crop_tile_kernel(const ResizeCropArgs a, int words_max, long long frame_bytes) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int t = threadIdx.x, tx = t % RC_TW, ty = t / RC_TW;
    const int n = blockIdx.z;
    const int oy0 = blockIdx.y * RC_TH, ox0 = blockIdx.x * RC_TW;
    const int oy1 = min(oy0 + RC_TH, a.oh) - 1, ox1 = min(ox0 + RC_TW, a.ow) - 1;  // last output row / col of the tile
    const int ys0 = (int)(((long long)(oy0 + a.y0) * a.H) / a.rh), ye1 = (int)((((long long)(oy1 + a.y0) + 1) * a.H + a.rh - 1) / a.rh);
    const int xs0 = (int)(((long long)(ox0 + a.x0) * a.W) / a.rw), xe1 = (int)((((long long)(ox1 + a.x0) + 1) * a.W + a.rw - 1) / a.rw);
    const int pitch = a.W * C * (int)sizeof(T);                 // bytes per source row (multiple of 4, checked by the launcher)
    const int b0 = (xs0 * C * (int)sizeof(T)) & ~3;             // staged byte range of a row: [b0, b0 + 4*words)
    const int words = (xe1 * C * (int)sizeof(T) - b0 + 3) >> 2;
    const int nrows = ye1 - ys0;
    const unsigned char* img = static_cast<const unsigned char*>(a.src) + (size_t)n * frame_bytes;
    const long long limit = (long long)(a.N - n) * frame_bytes;  // bytes from `img` to the end of the source buffer
    for (int i = t; i < nrows * words; i += 256) {
        const int r = i / words, wd = i - r * words;
        const long long off = (long long)(ys0 + r) * pitch + b0 + 4 * wd;
        uint32_t v;
        if (off + 4 <= limit) {
            v = *reinterpret_cast<const uint32_t*>(img + off);
        } else {  // the last word of the last row of the last frame may stick out of the buffer
            v = 0;
            for (int b = 0; b < 4; ++b)
                if (off + b < limit) v |= (uint32_t)img[off + b] << (8 * b);
        }
        lds[r * words_max + wd] = v;
    }
    __syncthreads();
    const int oy = oy0 + ty, ox = ox0 + tx;
    if (oy >= a.oh || ox >= a.ow) return;
    const int ry = oy + a.y0, rx = ox + a.x0;
    const int ys = (int)(((long long)ry * a.H) / a.rh), ye = (int)((((long long)ry + 1) * a.H + a.rh - 1) / a.rh);
    const int xs = (int)(((long long)rx * a.W) / a.rw), xe = (int)((((long long)rx + 1) * a.W + a.rw - 1) / a.rw);
    float sum[C];
#pragma unroll
    for (int c = 0; c < C; ++c) sum[c] = 0.f;
    const unsigned char* lb = reinterpret_cast<const unsigned char*>(lds);
    for (int y = ys; y < ye; ++y) {
        const T* row = reinterpret_cast<const T*>(lb + (size_t)(y - ys0) * words_max * 4 + (size_t)xs * C * sizeof(T) - b0);
        for (int x = xs; x < xe; ++x, row += C) {
#pragma unroll
            for (int c = 0; c < C; ++c) sum[c] = sum[c] + (float)row[c];
        }
    }
    const float kh = (float)(ye - ys), kw = (float)(xe - xs);
    T* out = static_cast<T*>(a.dst) + (((size_t)n * a.oh + oy) * a.ow + ox) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = PixCast<T>::from(__fdiv_rn(__fdiv_rn(sum[c], kh), kw));
}

// Which kernel runs a call.  ONE function decides, from what the call's source side fixes (pointer, dtype, shape, resized extent,
// mode) and the two environment switches; the launcher and hab_obs_resize_crop_form both ask it.
struct ResizeCropChoice {
    int form;
    int words_max;       // tile: LDS row pitch in dwords
    size_t lds_bytes;    // tile: dynamic LDS of the launch
};

template <class T, int C>
static bool tile_fits(const ResizeCropArgs& a, ResizeCropChoice& ch) {
    const long long pitch = (long long)a.W * C * sizeof(T);
    if (pitch % 4 || (reinterpret_cast<uintptr_t>(a.src) & 3) || a.N > 65535) return false;
    // upper bounds of the tile's source footprint
    const int rows_max = (int)(((long long)RC_TH * a.H + a.rh - 1) / a.rh) + 2;
    const int px_max = (int)(((long long)RC_TW * a.W + a.rw - 1) / a.rw) + 2;
    ch.words_max = (int)((px_max * C * sizeof(T) + 3) / 4) + 2;
    ch.lds_bytes = (size_t)rows_max * ch.words_max * 4;
    if (ch.lds_bytes > 48 * 1024) return false;
    // grid.y = tile rows of the window <= tile rows of the resized image: the bound does not depend on the crop
    return cdiv(a.rh, RC_TH) <= 65535;
}

// -> HAB_RESIZE_FORM_* or a negative HAB_ERR_*.  Uses a.src, a.N, a.H, a.W, a.C, a.rh, a.rw, a.mode only.
template <class T>
static int choose_resize_crop(const ResizeCropArgs& a, ResizeCropChoice& ch) {
    static const bool no_tile = hab_env_flag("HAB_OBS_NO_TILE");
    ch = ResizeCropChoice{HAB_RESIZE_FORM_GENERIC, 0, 0};
    if (a.C > 4) return HAB_ERR_UNSUPPORTED;
    if constexpr (std::is_same_v<T, uint8_t>) {
        static const bool no_rgb8 = hab_env_flag("HAB_OBS_NO_RGB8");
        const long long bytes = (long long)a.N * a.H * a.W * 3;
        // widest window = ceil(W / rw) + 1 pixels
        if (a.mode == HAB_RESIZE_AREA && a.C == 3 && !no_rgb8 && (a.W + a.rw - 1) / a.rw + 1 <= 4 && bytes % 4 == 0 &&
            (reinterpret_cast<uintptr_t>(a.src) & 3) == 0)
            return ch.form = HAB_RESIZE_FORM_RGB8;
    }
    if (a.mode == HAB_RESIZE_AREA && !no_tile) {
        bool fits = false;
        if (a.C == 1) fits = tile_fits<T, 1>(a, ch);
        else if (a.C == 3) fits = tile_fits<T, 3>(a, ch);
        else if (a.C == 4) fits = tile_fits<T, 4>(a, ch);
        if (fits) return ch.form = HAB_RESIZE_FORM_TILE;
    }
    return ch.form = HAB_RESIZE_FORM_GENERIC;
}

template <class T, int C>
static int tile_launch(const ResizeCropArgs& a, const ResizeCropChoice& ch, hipStream_t stream) {
    const long long frame_bytes = (long long)a.W * C * sizeof(T) * a.H;
    dim3 grid(cdiv(a.ow, RC_TW), cdiv(a.oh, RC_TH), a.N);
    obs_resize_crop_tile_kernel<T, C><<<grid, 256, ch.lds_bytes, stream>>>(a, ch.words_max, frame_bytes);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

// uint8 RGB, area mode, windows at most 4 pixels wide (down-scaling by < 3x: the 640x480 -> 256 case has 2-3 pixel windows).
// Integer sums of <= 16 bytes are exact in any order, so the ATen summation order does not matter here: a window row is fetched as
// four aligned dwords, byte-aligned with v_alignbyte, and the three channel sums of the row are three v_dot4_u32_u8 each with
// window-width dependent 0/1 byte weights (byte j*3 + c of the 12-byte row segment belongs to channel c of window pixel j).
// ~45 instructions per output pixel and no LDS / barrier, against ~110 with byte-wise LDS reads.
__global__ void __launch_bounds__(256) obs_resize_crop_rgb8_kernel(const ResizeCropArgs a, long long last_dword) {
    const long long total = (long long)a.N * a.oh * a.ow;
    const uint32_t* src = static_cast<const uint32_t*>(a.src);
    uint8_t* dst = static_cast<uint8_t*>(a.dst);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int ox = (int)(e % a.ow);
        long long r_ = e / a.ow;
        const int oy = (int)(r_ % a.oh);
        const int n = (int)(r_ / a.oh);
        const int ry = oy + a.y0, rx = ox + a.x0;
        const int ys = (int)(((long long)ry * a.H) / a.rh), ye = (int)((((long long)ry + 1) * a.H + a.rh - 1) / a.rh);
        const int xs = (int)(((long long)rx * a.W) / a.rw), xe = (int)((((long long)rx + 1) * a.W + a.rw - 1) / a.rw);
        const int kw = xe - xs;
        const uint32_t k1 = kw > 1, k2 = kw > 2, k3 = kw > 3;
        const uint32_t rw0 = 1u | (k1 << 24), rw1 = k2 << 16, rw2 = k3 << 8;
        const uint32_t gw0 = 1u << 8, gw1 = k1 | (k2 << 24), gw2 = k3 << 16;
        const uint32_t bw0 = 1u << 16, bw1 = k1 << 8, bw2 = k2 | (k3 << 24);
        uint32_t sr = 0, sg = 0, sb = 0;
        for (int y = ys; y < ye; ++y) {
            const long long addr = (((long long)n * a.H + y) * a.W + xs) * 3;
            const long long i0 = addr >> 2;
            const uint32_t off = (uint32_t)(addr & 3);
            const uint32_t d0 = src[i0];
            const uint32_t d1 = src[i0 + 1 < last_dword ? i0 + 1 : last_dword];
            const uint32_t d2 = src[i0 + 2 < last_dword ? i0 + 2 : last_dword];
            const uint32_t d3 = src[i0 + 3 < last_dword ? i0 + 3 : last_dword];
            const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, off);
            const uint32_t w1 = __builtin_amdgcn_alignbyte(d2, d1, off);
            const uint32_t w2 = __builtin_amdgcn_alignbyte(d3, d2, off);
            sr = __builtin_amdgcn_udot4(w0, rw0, sr, false); sr = __builtin_amdgcn_udot4(w1, rw1, sr, false); sr = __builtin_amdgcn_udot4(w2, rw2, sr, false);
            sg = __builtin_amdgcn_udot4(w0, gw0, sg, false); sg = __builtin_amdgcn_udot4(w1, gw1, sg, false); sg = __builtin_amdgcn_udot4(w2, gw2, sg, false);
            sb = __builtin_amdgcn_udot4(w0, bw0, sb, false); sb = __builtin_amdgcn_udot4(w1, bw1, sb, false); sb = __builtin_amdgcn_udot4(w2, bw2, sb, false);
        }
        const float kh = (float)(ye - ys), kwf = (float)kw;
        uint8_t* o = dst + (size_t)e * 3;
        o[0] = (uint8_t)__fdiv_rn(__fdiv_rn((float)sr, kh), kwf);
        o[1] = (uint8_t)__fdiv_rn(__fdiv_rn((float)sg, kh), kwf);
        o[2] = (uint8_t)__fdiv_rn(__fdiv_rn((float)sb, kh), kwf);
    }
}

template <class T>
static int launch_resize_crop(const ResizeCropArgs& a, hipStream_t stream) {
    ResizeCropChoice ch;
    const int form = choose_resize_crop<T>(a, ch);
    if (form < 0) return form;
    const long long total = (long long)a.N * a.oh * a.ow;
    if constexpr (std::is_same_v<T, uint8_t>) {
        if (form == HAB_RESIZE_FORM_RGB8) {
            const long long bytes = (long long)a.N * a.H * a.W * 3;
            int blocks = (int)cdivl(total, 256);
            if (blocks > 65536) blocks = 65536;
            obs_resize_crop_rgb8_kernel<<<blocks, 256, 0, stream>>>(a, bytes / 4 - 1);
            HAB_LAUNCH_CHECK();
            return HAB_OK;
        }
    }
    if (form == HAB_RESIZE_FORM_TILE) {
        if (a.C == 1) return tile_launch<T, 1>(a, ch, stream);
        if (a.C == 3) return tile_launch<T, 3>(a, ch, stream);
        return tile_launch<T, 4>(a, ch, stream);
    }
    int blocks = (int)cdivl(total, 256);
    if (blocks > 16384) blocks = 16384;
    obs_resize_crop_kernel<T, 4><<<blocks, 256, 0, stream>>>(a);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}


// ------------------------------------------------------------------------------------------------------------------------------------
// CubeMap2Equirect / CubeMap2Fisheye (N6).  Reference: habitat_baselines/common/obs_transformers.py:239-1199: stack of
// the six face sensors -> permute -> float -> (depth: * z-factor) -> F.grid_sample(bilinear, zeros, align_corners=True) against six
// precomputed grids -> view(...).sum(1) -> cast -> permute, eight launches and about seven full-size temporaries per sensor group.
// The six grids are disjoint (a pixel is assigned to the first face that sees its ray), so the sum has one non-zero term: the table
// holds that face and its grid coordinates, and ONE gather launch reads the six NHWC sensors where they lie and writes the output
// once in the sensor dtype.  One thread owns an output pixel (all channels) for a run of frames: the table entry, the four tap
// offsets and the four weights are computed once and reused over the run.  Neighbouring output pixels map to neighbouring texels of
// one face, so the reads are locally coherent without LDS.
//
// Arithmetic is ATen's grid_sampler_2d (fp32, contraction off): ix = ((gx + 1) / 2) * (W - 1); x0 = floor(ix), x1 = x0 + 1; weights
// (x1-ix)*(y1-iy), (ix-x0)*(y1-iy), (x1-ix)*(iy-y0), (ix-x0)*(iy-y0); result = sum over nw, ne, sw, se in that order of value * weight;
// a tap outside the face contributes nothing, and nothing outside the face is read: the address of such a tap is moved onto a texel
// of the face and the value is discarded (gx = +1 gives x1 = W: the last face of the last frame must not be read past its end).
// With a z-factor each tap value is first multiplied by zfactor[y_tap * W + x_tap] (the reference multiplies the batch before it
// samples).
struct ProjEntry { int32_t face; float gx, gy; };
static_assert(sizeof(ProjEntry) == 12, "table entry = {int32 face; float gx; float gy}");

constexpr int PROJ_MAX_SRC = 6;
struct ProjectArgs {
    const void* src[PROJ_MAX_SRC];
    void* dst;
    const ProjEntry* table;
    const float* zf;
    int n_src, N, H, W;
    int out_h, out_w;
    int frames_per_thread;
};

template <class T, int C>
struct PixIO {  // one pixel = C elements
    static __device__ void load(const T* p, float (&v)[C]) {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = (float)p[c];
    }
    static __device__ void store(T* p, const float (&v)[C]) {
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = PixCast<T>::from(v[c]);
    }
};

// What one output pixel needs of its face, the same for every frame: ATen's unnormalised coordinates, corner weights and bounds.
struct ProjTaps {
    float w[4];                      // nw, ne, sw, se
    bool okx0, okx1, oky0, oky1;     // column x0 / x1 and row y0 / y1 inside the face
    int xi0, xi1, yi0, yi1;          // the same as integers, 0 where outside (a texel of the face whose value is discarded)
};

__device__ inline ProjTaps proj_taps(float gx, float gy, int H, int W) {
    ProjTaps t;
    const float ix = ((gx + 1.f) / 2.f) * (float)(W - 1);
    const float iy = ((gy + 1.f) / 2.f) * (float)(H - 1);
    const float x0 = floorf(ix), y0 = floorf(iy), x1 = x0 + 1.f, y1 = y0 + 1.f;
    t.w[0] = (x1 - ix) * (y1 - iy); t.w[1] = (ix - x0) * (y1 - iy); t.w[2] = (x1 - ix) * (iy - y0); t.w[3] = (ix - x0) * (iy - y0);
    // bounds in the float domain: a NaN or huge coordinate fails every comparison and no tap is used
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    t.okx0 = x0 >= 0.f && x0 <= xmax; t.okx1 = x1 >= 0.f && x1 <= xmax;
    t.oky0 = y0 >= 0.f && y0 <= ymax; t.oky1 = y1 >= 0.f && y1 <= ymax;
    t.xi0 = t.okx0 ? (int)x0 : 0; t.xi1 = t.okx1 ? (int)x1 : 0; t.yi0 = t.oky0 ? (int)y0 : 0; t.yi1 = t.oky1 ? (int)y1 : 0;
    return t;
}

__device__ inline const void* proj_face(const ProjectArgs& a, int face) {
    const void* base = nullptr;  // select, not index: a runtime index into the by-value pointer array would put it in scratch
#pragma unroll
    for (int f = 0; f < PROJ_MAX_SRC; ++f)
        if (face == f) base = a.src[f];
    return base;
}

constexpr int PROJ_UNROLL = 4;  // frames in flight per thread
// A workgroup owns a 32 x 8 tile of output pixels: rows that are neighbours in the output read the same rows of the face, and inside
// one workgroup the second reader finds them in the CU's vector cache (row-major strips of 256 pixels put vertical neighbours on
// different XCDs, each of which fetched the face rows into its own L2).
constexpr int PROJ_TW = 32, PROJ_TH = 8;

// Any dtype and channel count: four taps, each read on its own.
template <class T, int C, bool ZF>
__global__ void __launch_bounds__(256) obs_project_kernel(const ProjectArgs a) {
    const int ox = blockIdx.x * PROJ_TW + threadIdx.x % PROJ_TW, oy = blockIdx.y * PROJ_TH + threadIdx.x / PROJ_TW;
    if (ox >= a.out_w || oy >= a.out_h) return;
    const int p = oy * a.out_w + ox, out_px = a.out_h * a.out_w;
    const int n0 = blockIdx.z * a.frames_per_thread;
    const int n1 = min(n0 + a.frames_per_thread, a.N);
    const size_t frame = (size_t)a.H * a.W * C;
    T* out = static_cast<T*>(a.dst) + ((size_t)n0 * out_px + p) * C;
    const size_t out_stride = (size_t)out_px * C;
    const ProjEntry e = a.table[p];
    float zero[C];
#pragma unroll
    for (int c = 0; c < C; ++c) zero[c] = 0.f;
    if (e.face < 0 || e.face >= a.n_src) {  // no source: 0 in every channel
        for (int n = n0; n < n1; ++n, out += out_stride) PixIO<T, C>::store(out, zero);
        return;
    }
    const ProjTaps t = proj_taps(e.gx, e.gy, a.H, a.W);
    const bool ok[4] = {t.okx0 && t.oky0, t.okx1 && t.oky0, t.okx0 && t.oky1, t.okx1 && t.oky1};
    const int tex[4] = {t.yi0 * a.W + t.xi0, t.yi0 * a.W + t.xi1, t.yi1 * a.W + t.xi0, t.yi1 * a.W + t.xi1};
    float z[4] = {1.f, 1.f, 1.f, 1.f};
    if (ZF) {
#pragma unroll
        for (int k = 0; k < 4; ++k) z[k] = a.zf[tex[k]];
    }
    const T* face = static_cast<const T*>(proj_face(a, e.face));
    for (int n = n0; n < n1; n += PROJ_UNROLL) {
        float v[PROJ_UNROLL][4][C];
#pragma unroll
        for (int u = 0; u < PROJ_UNROLL; ++u) {  // every load of the batch is issued before the first use; the tail repeats frame n1 - 1
            const T* img = face + (size_t)min(n + u, n1 - 1) * frame;
#pragma unroll
            for (int k = 0; k < 4; ++k) PixIO<T, C>::load(img + (size_t)tex[k] * C, v[u][k]);
        }
#pragma unroll
        for (int u = 0; u < PROJ_UNROLL; ++u) {
            if (n + u >= n1) break;
            float r[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                r[c] = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) r[c] = r[c] + (ok[k] ? (ZF ? v[u][k][c] * z[k] : v[u][k][c]) * t.w[k] : 0.f);
            }
            PixIO<T, C>::store(out + (size_t)(n + u - n0) * out_stride, r);
        }
    }
}

// The two flagship sensors, float32 depth (C = 1) and packed uint8 rgb (C = 3): the taps x0 and x1 of a row are neighbours in
// memory, so ONE load per row fetches both -- two loads per frame instead of four dword or twelve byte loads.  The pair starts at
// column xb = min(x0, W - 2) (0 when x0 is outside), so it lies inside the row also when x0 or x1 does not; which half holds x0 and
// which x1 is the same for every frame.
typedef float f32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));

template <class T>
struct PairFetch;
template <>
struct PairFetch<float> {  // dwordx2 at texel (y, xb)
    static constexpr int C = 1;
    int off;
    __device__ PairFetch(int y, int xb, int W, int) : off(y * W + xb) {}
    __device__ void load(const float* img, float (&px)[2][1]) const {
        const f32x2_a4 d = *reinterpret_cast<const f32x2_a4*>(img + off);
        px[0][0] = d.x; px[1][0] = d.y;
    }
};
template <>
struct PairFetch<uint8_t> {  // the six bytes of (y, xb), (y, xb + 1) inside three aligned dwords that do not leave the frame
    static constexpr int C = 3;
    int base;        // byte offset of the first dword inside the frame (frames are a multiple of 4 bytes, checked by the launcher)
    uint32_t shift;  // position of the first byte in the dwords, 0..6
    __device__ PairFetch(int y, int xb, int W, int frame_bytes) {
        const int addr = (y * W + xb) * 3;
        base = min(addr & ~3, frame_bytes - 12);
        shift = (uint32_t)(addr - base);
    }
    __device__ void load(const uint8_t* img, float (&px)[2][3]) const {
        const u32x3_a4 d = *reinterpret_cast<const u32x3_a4*>(img + base);
        const bool hi = shift >= 4;
        const uint32_t d0 = hi ? d.y : d.x, d1 = hi ? d.z : d.y;
        const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, shift & 3);   // bytes 0..3 of the pair
        const uint32_t w1 = __builtin_amdgcn_alignbyte(d.z, d1, shift & 3);  // bytes 4..5 (hi: shift & 3 <= 2, they come from d1)
        px[0][0] = (float)(w0 & 255u); px[0][1] = (float)((w0 >> 8) & 255u); px[0][2] = (float)((w0 >> 16) & 255u);
        px[1][0] = (float)(w0 >> 24); px[1][1] = (float)(w1 & 255u); px[1][2] = (float)((w1 >> 8) & 255u);
    }
};

template <class T, bool ZF>
__global__ void __launch_bounds__(256) obs_project_pair_kernel(const ProjectArgs a) {
    constexpr int C = PairFetch<T>::C;
    const int ox = blockIdx.x * PROJ_TW + threadIdx.x % PROJ_TW, oy = blockIdx.y * PROJ_TH + threadIdx.x / PROJ_TW;
    if (ox >= a.out_w || oy >= a.out_h) return;
    const int p = oy * a.out_w + ox, out_px = a.out_h * a.out_w;
    const int n0 = blockIdx.z * a.frames_per_thread;
    const int n1 = min(n0 + a.frames_per_thread, a.N);
    const int frame = a.H * a.W * C;
    T* out = static_cast<T*>(a.dst) + ((size_t)n0 * out_px + p) * C;
    const size_t out_stride = (size_t)out_px * C;
    const ProjEntry e = a.table[p];
    float zero[C];
#pragma unroll
    for (int c = 0; c < C; ++c) zero[c] = 0.f;
    if (e.face < 0 || e.face >= a.n_src) {
        for (int n = n0; n < n1; ++n, out += out_stride) PixIO<T, C>::store(out, zero);
        return;
    }
    const ProjTaps t = proj_taps(e.gx, e.gy, a.H, a.W);
    const bool ok[4] = {t.okx0 && t.oky0, t.okx1 && t.oky0, t.okx0 && t.oky1, t.okx1 && t.oky1};
    const int xb = t.okx0 ? min(t.xi0, a.W - 2) : 0;                   // W >= 2, checked by the launcher
    const bool s0 = t.okx0 && t.xi0 != xb, s1 = t.okx1 && t.xi1 != xb;  // x0 / x1 is the SECOND texel of the pair
    const PairFetch<T> f0(t.yi0, xb, a.W, frame * (int)sizeof(T)), f1(t.yi1, xb, a.W, frame * (int)sizeof(T));
    float z[4] = {1.f, 1.f, 1.f, 1.f};
    if (ZF) {
        const int tex[4] = {t.yi0 * a.W + t.xi0, t.yi0 * a.W + t.xi1, t.yi1 * a.W + t.xi0, t.yi1 * a.W + t.xi1};
#pragma unroll
        for (int k = 0; k < 4; ++k) z[k] = a.zf[tex[k]];
    }
    const T* face = static_cast<const T*>(proj_face(a, e.face));
    for (int n = n0; n < n1; n += PROJ_UNROLL) {
        float top[PROJ_UNROLL][2][C], bot[PROJ_UNROLL][2][C];
#pragma unroll
        for (int u = 0; u < PROJ_UNROLL; ++u) {  // every load of the batch is issued before the first use; the tail repeats frame n1 - 1
            const T* img = face + (size_t)min(n + u, n1 - 1) * frame;
            f0.load(img, top[u]);
            f1.load(img, bot[u]);
        }
#pragma unroll
        for (int u = 0; u < PROJ_UNROLL; ++u) {
            if (n + u >= n1) break;
            float r[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float v[4] = {s0 ? top[u][1][c] : top[u][0][c], s1 ? top[u][1][c] : top[u][0][c],
                                    s0 ? bot[u][1][c] : bot[u][0][c], s1 ? bot[u][1][c] : bot[u][0][c]};
                r[c] = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) r[c] = r[c] + (ok[k] ? (ZF ? v[k] * z[k] : v[k]) * t.w[k] : 0.f);
            }
            PixIO<T, C>::store(out + (size_t)(n + u - n0) * out_stride, r);
        }
    }
}

template <class T, int C>
static int launch_project_c(const ProjectArgs& a0, hipStream_t stream) {
    ProjectArgs a = a0;
    const int tiles_x = cdiv(a.out_w, PROJ_TW), tiles_y = cdiv(a.out_h, PROJ_TH);
    if (tiles_y > 65535) return HAB_ERR_UNSUPPORTED;
    // enough workgroups to fill the chip (about 8 per CU), then as many frames per thread as that leaves
    int chunks = (int)cdivl(2048, (long long)tiles_x * tiles_y);
    if (chunks > a.N) chunks = a.N;
    a.frames_per_thread = cdiv(a.N, chunks);
    chunks = cdiv(a.N, a.frames_per_thread);
    dim3 grid(tiles_x, tiles_y, chunks);
    const bool zf = a.zf != nullptr;
    if constexpr ((std::is_same_v<T, float> && C == 1) || (std::is_same_v<T, uint8_t> && C == 3)) {
        const long long frame_bytes = (long long)a.H * a.W * C * sizeof(T);
        bool aligned = (reinterpret_cast<uintptr_t>(a.dst) & 3) == 0;
        for (int f = 0; f < a.n_src; ++f) aligned = aligned && (reinterpret_cast<uintptr_t>(a.src[f]) & 3) == 0;
        if (a.W >= 2 && frame_bytes % 4 == 0 && frame_bytes >= 12 && aligned) {
            if (zf) obs_project_pair_kernel<T, true><<<grid, 256, 0, stream>>>(a);
            else obs_project_pair_kernel<T, false><<<grid, 256, 0, stream>>>(a);
            HAB_LAUNCH_CHECK();
            return HAB_OK;
        }
    }
    if (zf) obs_project_kernel<T, C, true><<<grid, 256, 0, stream>>>(a);
    else obs_project_kernel<T, C, false><<<grid, 256, 0, stream>>>(a);
    HAB_LAUNCH_CHECK();
    return HAB_OK;
}

template <class T>
static int launch_project(const ProjectArgs& a, int C, hipStream_t stream) {
    switch (C) {
    case 1: return launch_project_c<T, 1>(a, stream);
    case 2: return launch_project_c<T, 2>(a, stream);
    case 3: return launch_project_c<T, 3>(a, stream);
    case 4: return launch_project_c<T, 4>(a, stream);
    default: return HAB_ERR_ARG;
    }
}

}  // namespace hab

extern "C" int hab_obs_resize_crop(const void* src, void* dst, int dtype, int N, int H, int W, int C, int resized_h, int resized_w,
                                   int crop_y0, int crop_x0, int out_h, int out_w, int mode, hipStream_t stream) {
    using namespace hab;
    if (!src || !dst || N <= 0 || H <= 0 || W <= 0 || C <= 0 || resized_h <= 0 || resized_w <= 0 || out_h <= 0 || out_w <= 0)
        return HAB_ERR_ARG;
    if (crop_y0 < 0 || crop_x0 < 0 || crop_y0 + out_h > resized_h || crop_x0 + out_w > resized_w) return HAB_ERR_ARG;
    if (mode != HAB_RESIZE_AREA && mode != HAB_RESIZE_NEAREST) return HAB_ERR_ARG;
    ResizeCropArgs a{src, dst, N, H, W, C, resized_h, resized_w, crop_y0, crop_x0, out_h, out_w, mode};
    switch (dtype) {
    case HAB_DTYPE_U8: return launch_resize_crop<uint8_t>(a, stream);
    case HAB_DTYPE_F32: return launch_resize_crop<float>(a, stream);
    case HAB_DTYPE_I32: return launch_resize_crop<int32_t>(a, stream);
    default: return HAB_ERR_UNSUPPORTED;
    }
}


extern "C" int hab_obs_resize_crop_form(const void* src, int dtype, int N, int H, int W, int C, int resized_h, int resized_w, int mode) {
    using namespace hab;
    if (!src || N <= 0 || H <= 0 || W <= 0 || C <= 0 || resized_h <= 0 || resized_w <= 0) return HAB_ERR_ARG;
    if (mode != HAB_RESIZE_AREA && mode != HAB_RESIZE_NEAREST) return HAB_ERR_ARG;
    ResizeCropArgs a{src, nullptr, N, H, W, C, resized_h, resized_w, 0, 0, resized_h, resized_w, mode};
    ResizeCropChoice ch;
    switch (dtype) {
    case HAB_DTYPE_U8: return choose_resize_crop<uint8_t>(a, ch);
    case HAB_DTYPE_F32: return choose_resize_crop<float>(a, ch);
    case HAB_DTYPE_I32: return choose_resize_crop<int32_t>(a, ch);
    default: return HAB_ERR_UNSUPPORTED;
    }
}


extern "C" int hab_obs_project(const void* const* src, int n_src, void* dst, int dtype, int N, int H, int W, int C, const void* table,
                               const float* zfactor, int out_h, int out_w, hipStream_t stream) {
    using namespace hab;
    if (!src || !dst || !table || n_src < 1 || n_src > PROJ_MAX_SRC || N <= 0 || H <= 0 || W <= 0 || C < 1 || C > 4 || out_h <= 0 ||
        out_w <= 0)
        return HAB_ERR_ARG;
    for (int f = 0; f < n_src; ++f)
        if (!src[f]) return HAB_ERR_ARG;
    if (dtype != HAB_DTYPE_U8 && dtype != HAB_DTYPE_F32) return HAB_ERR_UNSUPPORTED;
    // texel offsets inside a face and the output pixel index are 32-bit in the kernel; frame offsets are 64-bit
    if ((long long)H * W * C > 0x7fffffffLL || (long long)out_h * out_w > 0x7fffff00LL) return HAB_ERR_UNSUPPORTED;
    ProjectArgs a{};
    for (int f = 0; f < n_src; ++f) a.src[f] = src[f];
    a.dst = dst;
    a.table = static_cast<const ProjEntry*>(table);
    a.zf = zfactor;
    a.n_src = n_src; a.N = N; a.H = H; a.W = W;
    a.out_h = out_h; a.out_w = out_w;
    return dtype == HAB_DTYPE_U8 ? launch_project<uint8_t>(a, C, stream) : launch_project<float>(a, C, stream);
}
