// resnet_ops.h -- argument blocks / launchers of the encoder-side HBM-bound kernels (resnet_ops.hip).
#pragma once
#include "hab_common.h"

namespace hab {

struct GnArgs {
    const float* x; float* y;           // [B][HW][C]
    const float* gamma; const float* beta;
    const float* residual;              // optional, added before the ReLU
    float* mean; float* rstd;           // [B][groups] saved for backward
    int B, HW, C, groups, relu;
    float eps;
    float* scratch = nullptr;           // optional: partial statistics of the chunk-parallel path for frames > 128 KB
    size_t scratch_floats = 0;          //   (>= B * ceil(HW*C / 16384) * groups * 2 floats), else the streaming kernel runs
};
struct GnBwdArgs {
    const float* x; const float* dy; const float* relu_out;  // relu_out: output of the fused ReLU (mask), or null
    float* dx;
    float* dy_masked;                   // optional: dy * (relu_out > 0) written out (gradient of the residual branch)
    const float* gamma; const float* mean; const float* rstd;
    float* chan_sums;                   // [B][2][C]: per-frame sum dy', sum dy'*xhat
    int B, HW, C, groups;
    float* scratch = nullptr;           // optional, >= B * ceil(HW*C / 8192) * 2 * C floats (chunk-parallel path)
    size_t scratch_floats = 0;
    // Stem form (groupnorm_relu_maxpool_forward): the layer's output went through ReLU + MaxPool2d(3, 2, 1) and was never stored.
    // dy is then GATHERED from the gradient of the pooled tensor (pool_dy [B][Ho][Wo][C], arg-max bytes pool_idx) and the ReLU mask is
    // recomputed from x, mean, rstd, gamma, beta with the forward's arithmetic; `dy` / `relu_out` are ignored.  Chunk-parallel path only.
    const float* pool_dy = nullptr; const uint8_t* pool_idx = nullptr; const float* beta = nullptr;
    int pH = 0, pW = 0;                 // spatial size of x (pooled: (pH + 1) / 2 x (pW + 1) / 2)
};
// 1-D sensor embeddings of PointNavResNetNet.forward (resnet_policy.py:662-753), each 32 wide, written side by side into
// the RNN input.  Slot kinds:
enum { EMB_POLAR = 0,   // pointgoal_with_gps_compass (rho, phi) -> Linear(3,32)([rho, cos(-phi), sin(-phi)])   :662-692
       EMB_TOKEN = 1,   // objectgoal id -> Embedding(n_categories, 32)                                          :715-717
       EMB_COSSIN = 2,  // compass x -> Linear(2,32)([cos x, sin x])                                             :719-729
       EMB_LIN2 = 3,    // gps (x, y) -> Linear(2,32)                                                            :731-734
       EMB_PREV = 4,    // previous action -> Embedding(A+1, 32)(mask ? a + 1 : 0)                               :747-753
       EMB_PREVLIN = 5,  // continuous previous action (A <= 4 floats) -> Linear(A, 32)(mask * a); ntok carries A      :754-757
       EMB_LINN = 6 };   // pointgoal (PointGoalSensor) / proximity: Linear(d, 32) on the raw d <= 4 floats; ntok carries d :694-700
constexpr int EMB_MAX_SLOTS = 7;
struct EmbedSlot {
    int kind;
    const void* in;      // sensor buffer (arena rows): f32 [rows][2] / int64 [rows][1] / f32 [rows][1] / f32 [rows][2] / int64 [rows][1]
    const float* w;      // Linear weight [32][nfeat] or embedding table [ntok][32]
    const float* b;      // Linear bias or null
    float* dw; float* db;  // gradients (backward only)
    int ntok;
};
__host__ __device__ inline int emb_nfeat(const EmbedSlot& sl) {
    return sl.kind == EMB_POLAR ? 3 : (sl.kind == EMB_COSSIN || sl.kind == EMB_LIN2) ? 2 : (sl.kind == EMB_PREVLIN || sl.kind == EMB_LINN) ? sl.ntok : 0;
}
struct EmbedArgs {
    EmbedSlot slot[EMB_MAX_SLOTS];
    int nslots;
    const uint8_t* masks; const int* rows;
    float* out; int ld, col0, B;
    float* saved;  // [B][nslots][4]: features / token (as float) -- kept for the backward pass
};
struct EmbedBwdArgs {
    EmbedSlot slot[EMB_MAX_SLOTS];
    int nslots;
    const float* saved;
    const float* dout; int ld, col0, B;
};

int ingest_pool(const uint8_t* rgb, const float* depth, const int32_t* semantic, const int* rows, float* y, int B, int H, int W, int cpad,
                int c_rgb, int c_depth, int c_sem, hipStream_t s, const float* norm_mean = nullptr, const float* norm_var = nullptr,
                const float* pivot = nullptr, double* mom_partial = nullptr, int* mom_blocks = nullptr);
// The visual sensors of a ResNetEncoder as a table (resnet_policy.py:178-199: every rank-3 observation, under any name, in concatenation
// order); travels to the ingest kernel by value.  vec[i]: the sensor's two horizontal taps may be fetched as one aligned unit (even W and
// an aligned base: uint8 x 3 as three 16-bit loads, float32 x 1 as one 8-byte load).
constexpr int INGEST_MAX_SENSORS = 4;
struct IngestTable {
    const void* src[INGEST_MAX_SENSORS];
    float scale[INGEST_MAX_SENSORS];                         // uint8: fp32(1 / high.max())
    signed char dtype[INGEST_MAX_SENSORS], ch[INGEST_MAX_SENSORS], off[INGEST_MAX_SENSORS], vec[INGEST_MAX_SENSORS];  // HAB_DTYPE_*, channels, first output channel
    int n;
};
constexpr int INGEST_U8 = 0, INGEST_F32 = 1, INGEST_I32 = 2;  // = HAB_DTYPE_* (checked in resnet_ops.hip)
// Fills off[] / vec[] and checks the table; *creal = total channels.
inline int ingest_table_finish(IngestTable& t, int W, int cpad, int* creal) {
    if (t.n <= 0 || t.n > INGEST_MAX_SENSORS || (cpad != 4 && cpad != 8)) return HAB_ERR_ARG;
    int off = 0;
    for (int i = 0; i < t.n; ++i) {
        const int dt = t.dtype[i], C = t.ch[i];
        if (!t.src[i] || C <= 0 || C > 8 || (dt != INGEST_U8 && dt != INGEST_F32 && dt != INGEST_I32)) return HAB_ERR_ARG;
        t.off[i] = (signed char)off;
        off += C;
        if (off > cpad) return HAB_ERR_ARG;
        const uintptr_t a = reinterpret_cast<uintptr_t>(t.src[i]);
        t.vec[i] = 0;
        if (!(W & 1)) {
            if (dt == INGEST_U8 && C == 3 && !(a & 1)) t.vec[i] = 1;
            if (dt == INGEST_F32 && C == 1 && !(a & 7)) t.vec[i] = 1;
        }
        if (dt != INGEST_U8) t.scale[i] = 1.f;
    }
    if (creal) *creal = off;
    return HAB_OK;
}
__host__ __device__ __forceinline__ void ingest_put(float (&out)[8], int k, float v) {
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (c == k) out[c] = v;   // select chain: out[] stays in registers
}
// One output pixel of the table-driven ingest: out[0 .. 8) = the concatenated channels (zeros behind the last sensor).  px: pixel index of
// tap (0,0) in a sensor's (rows, H, W) plane; (0,1) = px + 1, (1,0) = px + W, (1,1) = px + W + 1.  Host-callable so that the CPU suite pins
// the arithmetic and the byte unpacking without a GPU (tests/hostcheck/hostcheck_ingest.hip).
__host__ __device__ __forceinline__ void ingest_table_pixel(const IngestTable& t, size_t px, int W, float (&out)[8]) {
#pragma clang fp contract(off)  // the reference rounds the uint8 scaling and every addition of the 2x2 average separately
#pragma unroll
    for (int c = 0; c < 8; ++c) out[c] = 0.f;
#pragma unroll
    for (int i = 0; i < INGEST_MAX_SENSORS; ++i) {
        if (i >= t.n) break;
        const int C = t.ch[i], c0 = t.off[i], dt = t.dtype[i];
        if (dt == INGEST_U8) {
            const uint8_t* p = static_cast<const uint8_t*>(t.src[i]);
            const float sc = t.scale[i];
            if (C == 3 && t.vec[i]) {
                const uint16_t* r0 = reinterpret_cast<const uint16_t*>(p + px * 3);
                const uint16_t* r1 = reinterpret_cast<const uint16_t*>(p + (px + W) * 3);
                const unsigned a0 = r0[0], a1 = r0[1], a2 = r0[2], b0 = r1[0], b1 = r1[1], b2 = r1[2];
                // bytes of a row: tap 0 = (a0 & 255, a0 >> 8, a1 & 255), tap 1 = (a1 >> 8, a2 & 255, a2 >> 8)
                const unsigned t00[3] = {a0 & 255u, a0 >> 8, a1 & 255u}, t01[3] = {a1 >> 8, a2 & 255u, a2 >> 8};
                const unsigned t10[3] = {b0 & 255u, b0 >> 8, b1 & 255u}, t11[3] = {b1 >> 8, b2 & 255u, b2 >> 8};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float s = 0.f;
                    s = s + (float)t00[c] * sc; s = s + (float)t01[c] * sc; s = s + (float)t10[c] * sc; s = s + (float)t11[c] * sc;
                    ingest_put(out, c0 + c, s * 0.25f);
                }
            } else {
                for (int c = 0; c < C; ++c) {
                    float s = 0.f;
                    s = s + (float)p[px * C + c] * sc; s = s + (float)p[(px + 1) * C + c] * sc;
                    s = s + (float)p[(px + W) * C + c] * sc; s = s + (float)p[(px + W + 1) * C + c] * sc;
                    ingest_put(out, c0 + c, s * 0.25f);
                }
            }
        } else if (dt == INGEST_F32) {
            const float* p = static_cast<const float*>(t.src[i]);
            if (C == 1 && t.vec[i]) {
                const float2 u = *reinterpret_cast<const float2*>(p + px), v = *reinterpret_cast<const float2*>(p + px + W);
                float s = 0.f;
                s = s + u.x; s = s + u.y; s = s + v.x; s = s + v.y;
                ingest_put(out, c0, s * 0.25f);
            } else {
                for (int c = 0; c < C; ++c) {
                    float s = 0.f;
                    s = s + p[px * C + c]; s = s + p[(px + 1) * C + c]; s = s + p[(px + W) * C + c]; s = s + p[(px + W + 1) * C + c];
                    ingest_put(out, c0 + c, s * 0.25f);
                }
            }
        } else {  // int32 ids are concatenated by type promotion (torch.cat) and averaged like any channel
            const int32_t* p = static_cast<const int32_t*>(t.src[i]);
            for (int c = 0; c < C; ++c) {
                float s = 0.f;
                s = s + (float)p[px * C + c]; s = s + (float)p[(px + 1) * C + c];
                s = s + (float)p[(px + W) * C + c]; s = s + (float)p[(px + W + 1) * C + c];
                ingest_put(out, c0 + c, s * 0.25f);
            }
        }
    }
}
// The ingest of a sensor table: the legacy triple (at most one uint8 x 3 sensor scaled by 1/255, one float32 x 1, one int32 x 1) keeps its
// three-pointer kernel, every other table runs the table-driven one; same arithmetic, same moments / normalisation contract.
int ingest_pool_sensors(const IngestTable& t, const int* rows, float* y, int B, int H, int W, int cpad, hipStream_t s,
                        const float* norm_mean = nullptr, const float* norm_var = nullptr, const float* pivot = nullptr,
                        double* mom_partial = nullptr, int* mom_blocks = nullptr, bool force_table_kernel = false);
// fused moments of the ingest (training-mode RunningMeanAndVar): mom_partial holds [<= INGEST_MOM_MAX_BLOCKS][16] doubles
constexpr int INGEST_MOM_MAX_BLOCKS = 2048;
int moment_finish_mean(const double* partial, int nblocks, int cpad, const float* pivot, int creal, long long npix, double* sums,
                       float* mean_out, float* count_out, float count_val, hipStream_t s);
int moment_finish_var(const double* sums, const float* pivot, int creal, int cpad, const float* mean_sum, float mean_div, long long npix,
                      float* var_out, hipStream_t s);
int chan_moment(const float* x, long long npix, int cpad, int mode, const float* mean, float* out, double* scratch, int scratch_len,
                hipStream_t s, float mean_div = 1.f, float* count_out = nullptr, float count_val = 0.f);
int rmv_update(float* r_mean, float* r_var, float* r_count, const float* b_mean, const float* b_var, float n, int C, hipStream_t s,
               const float* n_dev = nullptr, float div = 1.f, float* aff = nullptr);
int rmv_normalize(float* x, long long npix, int cpad, int C, const float* mean, const float* var, hipStream_t s);
// conv_gn_ops.hip -- convolution (bias-free) + GroupNorm (+ residual, + ReLU) in one launch for the small-batch passes (conv_gn_slab.h)
struct ConvGnArgs {
    const float* x;                 // [B][H][W][C]
    const unsigned short* w_planes; // forward-packed weight [Cout][KH*KW*C] as three fragment-ordered bf16 planes (weight_planes)
    const float* gamma; const float* beta; const float* residual;
    float* y;
    float* raw = nullptr; float* mean = nullptr; float* rstd = nullptr;  // kept for a backward pass when given
    int B, H, W, C, Cout, KH, KW, stride, pad, groups, relu;
    float eps;
};
int conv_gn_fused_ok(int C, int Cout, int H, int W, int KH, int KW, int stride, int pad, int groups);
int weight_planes(const float* w, int Cout, int K, unsigned short* planes, hipStream_t s);  // fragment-ordered bf16 planes of the exact split
int conv_gn_fused(const ConvGnArgs& a, hipStream_t s);  // HAB_NOT_APPLICABLE: geometry not covered
// stem convolution 7x7 / 2 / 3, 4 -> 32 channels with the input strip resident in LDS (stem_conv_strip.h)
constexpr int STEM_PLANE_FLOATS = 3 * 14 * 1024 / 4;  // fragment-ordered bf16 planes of the filter, in floats of the packed arena
int stem_conv_ok(int H, int W, int C, int Cout, int KH, int KW, int stride, int pad);
int stem_weight_planes(const float* wf, unsigned short* planes, hipStream_t s);
int stem_conv_forward(const float* x, const unsigned short* planes, float* y, int B, int H, int W, hipStream_t s, const float* norm = nullptr,
                      float* gn_part = nullptr, int gn_groups = 0);  // gn_part: [B][ceil(Ho / STEM_STAT_ROWS)][groups][2] partial statistics
constexpr int STEM_STAT_ROWS = 8;  // HAB_NOT_APPLICABLE: not covered
// its weight gradient, both operands resident in LDS, transpose reads (stem_wgrad_strip.h); ws >= 256 * 7 * 1024 floats; HAB_NOT_APPLICABLE: not covered
int stem_conv_wgrad(const float* x, const float* dy, float* dw_oihw, int B, int H, int W, int creal, float* ws, size_t ws_floats, hipStream_t s,
                    const float* norm = nullptr);
int stem_wgrad_ok(int H, int W, int C, int Cout, int KH, int KW, int stride, int pad);
int groupnorm_forward(const GnArgs& a, hipStream_t s);
int groupnorm_backward(const GnBwdArgs& a, hipStream_t s);
// GroupNorm + ReLU + MaxPool2d(3, 2, 1) in one pass over the GroupNorm input; the normalised frame is never written.  idx (nullable):
// arg-max bytes for the backward pass; a.mean / a.rstd (nullable) are written when given.  1: frame not on the chunk-parallel path.
int groupnorm_relu_maxpool_forward(const GnArgs& a, int H, int W, float* pool, uint8_t* idx, hipStream_t s, const float* ext_part = nullptr,
                                   int ext_rows = 0);
bool groupnorm_pool_fusable(int B, int HW, int C, int groups, size_t scratch_floats);  // forward AND backward chunk-parallel forms exist
int groupnorm_relu_materialize(const GnArgs& a, hipStream_t s);  // y = relu(GroupNorm(x)) from the SAVED a.mean / a.rstd (debug taps)
int maxpool_forward(const float* x, float* y, uint8_t* idx, int B, int H, int W, int C, hipStream_t s);
int maxpool_backward(const float* dy, const uint8_t* idx, float* dx, int B, int H, int W, int C, hipStream_t s);
// Squeeze-and-excitation gate of SEBottleneck (resnet.py:92-113,155-187): pooled[b][c] = mean_hw x;  y = relu(gate[b][c] * x + residual);
// backward pieces: dm = dy * (y > 0) (written out: it is also the residual branch's gradient), dgate[b][c] = sum_hw dm * x, and
// dx = dm * gate[b][c] + dpool[b][c] / HW (the squeeze's gradient spread over the frame).
int se_pool(const float* x, float* pooled, int B, int HW, int C, hipStream_t s);
int se_apply_forward(const float* x, const float* gate, const float* residual, float* y, int B, int HW, int C, hipStream_t s);
int se_backward_reduce(const float* dy, const float* y, const float* x, float* dm, float* dgate, int B, int HW, int C, hipStream_t s);
int se_backward_apply(const float* dm, const float* gate, const float* dpool, float* dx, int B, int HW, int C, hipStream_t s);
int sigmoid_inplace(float* z, long long n, hipStream_t s);
int sigmoid_grad(const float* g, const float* dg, float* dz, long long n, hipStream_t s);
// Grouped 3x3 convolution of the ResNeXt bottlenecks (resnet.py:72-89, groups = cardinality): the weight (Cout, Cin/groups, KH, KW)
// is expanded to the dense block-diagonal kernel layouts (zeros off the diagonal) so that the dense contraction kernels serve it;
// the dense weight gradient is computed into scratch and its block diagonal is gathered back.
int repack_conv_grouped(const float* w, float* wf, float* wd, int Cout, int Cin, int groups, int KH, int KW, hipStream_t s);
int gather_grouped_wgrad(const float* dense_oihw, float* dw, int Cout, int Cin, int groups, int KH, int KW, hipStream_t s);
int embed_forward(const EmbedArgs& a, hipStream_t s);
int embed_backward(const EmbedBwdArgs& a, float* ws, size_t ws_floats, hipStream_t s);

}  // namespace hab
